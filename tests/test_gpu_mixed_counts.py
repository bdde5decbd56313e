"""The mixed kernels at the counts where their indexing changes (tests/mixed_counts.py; held to these claims on the CPU by
tests/test_mixed_counts.py and tests/test_xcd_grids.py):

  * 65535 groups, the last launch xcd_map_for permutes (sets ON, ON_RAGGED), and 65537 groups, past the switch (set OFF),
    with a frame of 71 units across group 65408 where the permuted part ends;
  * fix-up ids unit * 64 + lane up to and past 2^24;
  * HVC_HUFF_MIXED_MAX_FILES = 65535 files in one launch of the mixed coder, the 65536th refused, 65537 in two chunks;
  * more than HVC_HDM_MAX_TABLE_SETS = 512 Huffman table sets in one chunk of the mixed reader.

Every comparison is exact equality against the CPU definitions the mixed modules use (oracle/orc.py, tools/scaled_reference.py,
tools/libjpeg_reference.py, the host coders, the host reader).  Every output buffer is filled with 0xA5, has a guard region
behind the last record and is compared whole: a unit nobody ran, a unit run twice with a neighbour's descriptor and a store
past the end all show.

Device memory only for the block stage: the host-memory form copies every frame by itself in both directions (stage_coefs,
decode_frames_mixed_impl) -- hundreds of thousands of copies at these counts -- and is covered at small counts by the mixed
modules."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import mixed_counts as mc
import test_gpu_mixed_libjpeg as tml
import test_gpu_mixed_scaled as tms
import xcd_grids as xg
from helpers import synth_coefs
from oracle import orc
from test_gpu_xcd_order import outside_the_model_guard, table_pair, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import libjpeg_reference as lj  # noqa: E402
import scaled_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL16 = np.int16(0xA5A5 - 0x10000)
GUARD = 4096                 # bytes / elements of fill behind the last record
T, D = mc.TABLES, mc.D


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd
    return video_coding_amd


@pytest.fixture()
def ctx(hvc):
    c = hvc.Context(0)
    yield c
    c.close()


def make_info(hvc, planes, tables, side=8, pad=0):
    """planes: (blocks_w, blocks_h, table index) each, tight coefficient planes, pixel planes of side x side samples a block with
    rows `pad` bytes wider than the plane, one behind the other"""
    info = hvc.hvc.JpegInfo()
    info.n_comp, info.n_qtabs = len(planes), len(tables)
    for t, q in enumerate(tables):
        for k in range(64):
            info.qtabs[t][k] = int(q[k])
    co = po = 0
    for i, (bw, bh, qt) in enumerate(planes):
        L = info.layout[i]
        L.blocks_w, L.blocks_h, L.qtab, L.coef_offset, L.plane_offset, L.stride = bw, bh, qt, co, po, bw * side + pad
        co += bw * bh * 64
        po += L.stride * bh * side
    info.coef_count, info.pixel_bytes = co, po
    return info


def blocks_of(planes):
    return sum(bw * bh for bw, bh, _ in planes)


def special_tables(s, pairs):
    """the table pair of every special: by its place among them"""
    return {f: pairs(k) for k, f in enumerate(sorted(s.special))}


def first_difference(s, got, want, offsets):
    """for the assertion message: the first byte / element that differs and the frame whose record holds or follows it"""
    if got.shape != want.shape:
        return "shapes %s / %s" % (got.shape, want.shape)
    at = np.flatnonzero(got != want)
    if not at.size:
        return None
    f = int(np.searchsorted(offsets, at[0], side="right")) - 1
    return "%d differ, the first at %d: frame %d (%s, first unit %d) + %d; got %d, want %d" % (
        at.size, at[0], f, s.special.get(f, "grey1"), s.unit0[max(f, 0)], at[0] - offsets[max(f, 0)], got[at[0]], want[at[0]])


# ---- the block stage to planes: k_decode_mixed + k_decode_mixed_wide --------------------------------------------------------
def model_grey():
    """(B [T][D][64] records the encoder makes under table t, W [T][D][64] their pixels by the oracle)"""
    B = np.stack([synth_coefs(9100 + t, D, 1, table_pair(t)[0])[0].reshape(D, 64) for t in range(T)])
    W = np.stack([orc.dequant_idct_recon(np.ascontiguousarray(B[t]).reshape(-1), table_pair(t)[0], 1, D).reshape(D, 64) for t in range(T)])
    return B, W


_CASES = {}


def decode_case(hvc, name, planted):
    """the set `name` for hvc_decode_frames_mixed -> dict(s, infos, coefs, co, po, want (the whole pixel buffer), wide); planted:
    the blocks of s.guard_places() dense +-2047.  The host arrays are kept for the module (50 MB a set); the descriptors are
    made per call"""
    key = ("decode", name, planted)
    if key not in _CASES:
        s = mc.count_set(name)
        B, W = model_grey()
        tabs = special_tables(s, table_pair)
        rng = np.random.default_rng(5)
        rec, want, wide = {}, {}, 0
        for f in s.special:
            planes, parts = s.planes(f), []
            for i, (bw, bh, t) in enumerate(planes):
                c = synth_coefs(9200 + 7 * f % 1000 + i, bh, bw, tabs[f][t])[0].copy().reshape(-1, 64) if bw * bh else np.zeros((0, 64), np.int16)
                if planted:
                    for pf, pp, pb in s.guard_places():
                        if (pf, pp) == (f, i):
                            c[pb] = rng.choice(np.array([-2047, 2047], dtype=np.int16), size=64)
                            assert outside_the_model_guard(c[pb], tabs[f][t]).all(), (pf, pp, pb)   # it really fails the packed guard
                if bw * bh:
                    wide += int(np.count_nonzero(outside_the_model_guard(c, tabs[f][t])))
                parts.append(c)
            rec[f] = np.concatenate(parts).reshape(-1)
            want[f] = np.concatenate([orc.dequant_idct_recon(np.ascontiguousarray(c).reshape(-1), tabs[f][t], bw, bh).reshape(-1)
                                      for c, (bw, bh, t) in zip(parts, planes) if bw * bh])
        for t in range(T):                                    # the tiled records are ordinary: none of them is counted
            assert not outside_the_model_guard(B[t], table_pair(t)[0]).any()
        assert wide == (len(s.guard_places()) if planted else 0)
        co, cend = mc.place(s, 64, lambda f: rec[f].size, align=8)
        po, pend = mc.place(s, 64, lambda f: want[f].size, align=8)
        coefs = np.zeros(cend + 64, dtype=np.int16)
        mc.fill(s, coefs, co, 64, lambda f: B[f % T, f % D], lambda f: rec[f])
        expect = np.full(pend + GUARD, FILL, dtype=np.uint8)
        mc.fill(s, expect, po, 64, lambda f: W[f % T, f % D], lambda f: want[f])
        _CASES[key] = dict(s=s, tabs=tabs, coefs=coefs, co=co, po=po, want=expect, wide=wide)
    case = dict(_CASES[key])
    s, tabs = case["s"], case["tabs"]
    case["infos"] = mc.descriptors(hvc.hvc.JpegInfo, s, [make_info(hvc, xg.MIXED_SHAPES["grey1"], table_pair(t)) for t in range(T)],
                                   lambda f: make_info(hvc, s.planes(f), tabs[f]))
    return case


def run_decode(ctx, case):
    d_c, d_p = to_device(case["coefs"], np.full(case["want"].size, FILL, dtype=np.uint8))
    ctx.decode_frames_mixed(d_c, mc.size_array(case["co"]), case["infos"], d_p, mc.size_array(case["po"]))
    ctx.synchronize()
    return d_p.cpu().numpy()


@pytest.mark.parametrize("name", ["ON", "ON_RAGGED", "OFF"])
def test_decode_frames_mixed(hvc, ctx, name):
    """65535 groups under the permutation, the last one full and with two spare units; 65537 groups as dispatched"""
    case = decode_case(hvc, name, False)
    assert case["s"].groups == mc.GROUPS[name] and (xg.xcd_map_for(case["s"].groups, 1) > 0) == (name != "OFF")
    got = run_decode(ctx, case)
    assert np.array_equal(got, case["want"]), first_difference(case["s"], got, case["want"], case["po"])
    assert ctx.last_wide_blocks() == 0


@pytest.mark.parametrize("name", ["ON", "OFF"])
def test_decode_frames_mixed_fix_up_ids(hvc, ctx, name):
    """k_decode_mixed_wide takes ids up to 2^24 - 313 (ON) and 2^24 + 71 (OFF) apart again: blocks outside the int32 guard in the
    first unit, on either side of group 65408, in the last unit, in lane 63"""
    case = decode_case(hvc, name, True)
    got = run_decode(ctx, case)
    assert np.array_equal(got, case["want"]), first_difference(case["s"], got, case["want"], case["po"])
    assert ctx.last_wide_blocks() == case["wide"] == len(case["s"].guard_places()) == 7


# ---- the scaled block stage: k_decode_mixed_scaled<N> ------------------------------------------------------------------------
_SCALED = {}


def scaled_records(name):
    """the records of the scaled tests: tests/test_gpu_mixed_scaled.py's ordinary blocks"""
    if name not in _SCALED:
        s = mc.count_set(name)
        tabs = special_tables(s, table_pair)
        B = np.stack([tms.ordinary_blocks(9300 + t, D) for t in range(T)])
        rec = {f: [tms.ordinary_blocks(9400 + 7 * f % 1000 + i, bw * bh) for i, (bw, bh, _) in enumerate(s.planes(f))] for f in s.special}
        co, cend = mc.place(s, 64, lambda f: 64 * blocks_of(s.planes(f)), align=8)
        coefs = np.zeros(cend + 64, dtype=np.int16)
        mc.fill(s, coefs, co, 64, lambda f: B[f % T, f % D], lambda f: np.concatenate(rec[f]).reshape(-1))
        _SCALED[name] = (s, tabs, B, rec, co, coefs)
    return _SCALED[name]


@pytest.mark.parametrize("name", ["ON", "OFF"])
@pytest.mark.parametrize("scale", tms.SCALES)
def test_decode_frames_mixed_scaled(hvc, ctx, scale, name):
    """tight records of n x n bytes a block one behind the other from byte 8: at 1/8 a one-block frame is one byte"""
    n = 8 // scale
    s, tabs, B, rec, co, coefs = scaled_records(name)
    W = np.stack([sr.scaled_plane(B[t], table_pair(t)[0], 1, D, n).reshape(D, n * n) for t in range(T)])
    wide_grey = np.stack([~sr.takes_int32_path(B[t], table_pair(t)[0], n) for t in range(T)])
    frames = np.array([f for f in range(s.n) if f not in s.special])
    wide = int(wide_grey[frames % T, frames % D].sum())
    want = {}
    for f in s.special:
        parts = []
        for b, (bw, bh, t) in zip(rec[f], s.planes(f)):
            if bw * bh:
                parts.append(sr.scaled_plane(b, tabs[f][t], bw, bh, n).reshape(-1))
                wide += int(np.count_nonzero(~sr.takes_int32_path(b, tabs[f][t], n)))
        want[f] = np.concatenate(parts)
    po, pend = mc.place(s, n * n, lambda f: want[f].size, lead=8)
    expect = np.full(pend + GUARD, FILL, dtype=np.uint8)
    mc.fill(s, expect, po, n * n, lambda f: W[f % T, f % D], lambda f: want[f])
    infos = mc.descriptors(hvc.hvc.JpegInfo, s, [make_info(hvc, xg.MIXED_SHAPES["grey1"], table_pair(t), n) for t in range(T)],
                           lambda f: make_info(hvc, s.planes(f), tabs[f], n))
    d_c, d_p = to_device(coefs, np.full(expect.size, FILL, dtype=np.uint8))
    ctx.decode_frames_mixed_scaled(d_c, mc.size_array(co), infos, scale, d_p, mc.size_array(po))
    ctx.synchronize()
    got = d_p.cpu().numpy()
    assert np.array_equal(got, expect), first_difference(s, got, expect, po)
    assert ctx.last_wide_blocks() == wide


# ---- the libjpeg-exact block stage: k_islow_mixed ----------------------------------------------------------------------------
def libjpeg_pair(k):
    return tml.ordinary_tables(20 + k % 3)


def libjpeg_blocks(seed, nblk):
    """tests/test_gpu_mixed_libjpeg.py's ordinary records: sparse small coefficients"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-30, 31, size=(nblk, 64)) * (rng.random(size=(nblk, 64)) < 0.3)
    c[:, 0] = rng.integers(-80, 81, size=nblk)
    return c.astype(np.int16)


@pytest.mark.parametrize("name", ["ON", "OFF"])
def test_decode_frames_mixed_libjpeg(hvc, ctx, name):
    """hvc_set_mixed_arithmetic("libjpeg"); the set without the empty component"""
    s = mc.count_set(name, zero=False)
    assert s.units == mc.UNITS[name]
    tabs = special_tables(s, libjpeg_pair)
    B = np.stack([libjpeg_blocks(9500 + t, D) for t in range(T)])
    W = np.stack([lj.islow_plane(B[t], libjpeg_pair(t)[0], 1, D).reshape(D, 64) for t in range(T)])
    wide_grey = np.stack([~lj.takes_int32_path(B[t], libjpeg_pair(t)[0]) for t in range(T)])
    frames = np.array([f for f in range(s.n) if f not in s.special])
    wide = int(wide_grey[frames % T, frames % D].sum())
    rec, want = {}, {}
    for f in s.special:
        blocks = [libjpeg_blocks(9600 + 7 * f % 1000 + i, bw * bh) for i, (bw, bh, _) in enumerate(s.planes(f))]
        rec[f] = np.concatenate(blocks).reshape(-1)
        want[f] = np.concatenate([lj.islow_plane(b, tabs[f][t], bw, bh).reshape(-1) for b, (bw, bh, t) in zip(blocks, s.planes(f))])
        wide += sum(int(np.count_nonzero(~lj.takes_int32_path(b, tabs[f][t]))) for b, (bw, bh, t) in zip(blocks, s.planes(f)))
    co, cend = mc.place(s, 64, lambda f: rec[f].size, align=8)
    po, pend = mc.place(s, 64, lambda f: want[f].size, align=8)
    coefs = np.zeros(cend + 64, dtype=np.int16)
    mc.fill(s, coefs, co, 64, lambda f: B[f % T, f % D], lambda f: rec[f])
    expect = np.full(pend + GUARD, FILL, dtype=np.uint8)
    mc.fill(s, expect, po, 64, lambda f: W[f % T, f % D], lambda f: want[f])
    infos = mc.descriptors(hvc.hvc.JpegInfo, s, [make_info(hvc, xg.MIXED_SHAPES["grey1"], libjpeg_pair(t)) for t in range(T)],
                           lambda f: make_info(hvc, s.planes(f), tabs[f]))
    ctx.set_mixed_arithmetic("libjpeg")
    d_c, d_p = to_device(coefs, np.full(expect.size, FILL, dtype=np.uint8))
    ctx.decode_frames_mixed(d_c, mc.size_array(co), infos, d_p, mc.size_array(po))
    ctx.synchronize()
    got = d_p.cpu().numpy()
    assert np.array_equal(got, expect), first_difference(s, got, expect, po)
    assert ctx.last_wide_blocks() == wide


# ---- the encoder's block stage: k_encode_mixed -------------------------------------------------------------------------------
PAD = 8                      # pixel rows this much wider than the plane
GAP = 8                      # elements of fill between two coefficient records (16 bytes: the next record stays on 16)


def pixel_rows(seed, rows, width):
    """noise in the even block rows, smooth content (small coefficients) in the odd ones"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, size=(rows, width), dtype=np.uint8)
    smooth = rng.integers(100, 140, size=(rows, width), dtype=np.uint8)
    odd = (np.arange(rows) // 8) % 2 == 1
    p[odd] = smooth[odd]
    return p


@pytest.mark.parametrize("name", ["ON", "OFF"])
def test_encode_frames_mixed(hvc, ctx, name):
    """pixel records to coefficient records against orc.fdct_quant; the coefficient records lie GAP elements of fill apart"""
    s = mc.count_set(name, zero=False)
    tabs = special_tables(s, table_pair)
    row = 8 + PAD
    P = np.stack([pixel_rows(9700 + t, 8 * D, row).reshape(D, 8 * row) for t in range(T)])
    W = np.stack([orc.fdct_quant(np.ascontiguousarray(P[t]).reshape(-1), table_pair(t)[0], 1, D, stride=row).reshape(D, 64) for t in range(T)])
    pix, want = {}, {}
    for f in s.special:
        planes = s.planes(f)
        parts = [pixel_rows(9800 + 7 * f % 1000 + i, 8 * bh, 8 * bw + PAD).reshape(-1) for i, (bw, bh, _) in enumerate(planes)]
        pix[f] = np.concatenate(parts)
        want[f] = np.concatenate([orc.fdct_quant(p, tabs[f][t], bw, bh, stride=8 * bw + PAD).reshape(-1) for p, (bw, bh, t) in zip(parts, planes)])
    po, pend = mc.place(s, 8 * row, lambda f: pix[f].size, align=64)
    co, cend = mc.place(s, 64 + GAP, lambda f: want[f].size + GAP, align=8)
    pixels = np.zeros(pend + 64, dtype=np.uint8)
    mc.fill(s, pixels, po, 8 * row, lambda f: P[f % T, f % D], lambda f: pix[f])
    expect = np.full(cend + GUARD, FILL16, dtype=np.int16)
    mc.fill(s, expect, co, 64 + GAP, lambda f: W[f % T, f % D], lambda f: want[f])
    infos = mc.descriptors(hvc.hvc.JpegInfo, s, [make_info(hvc, xg.MIXED_SHAPES["grey1"], table_pair(t), pad=PAD) for t in range(T)],
                           lambda f: make_info(hvc, s.planes(f), tabs[f], pad=PAD))
    d_p, d_c = to_device(pixels, np.full(expect.size, FILL16, dtype=np.int16))
    ctx.encode_frames_mixed(d_p, mc.size_array(po), infos, d_c, mc.size_array(co))
    ctx.synchronize()
    got = d_c.cpu().numpy()
    assert np.array_equal(got, expect), first_difference(s, got, expect, co)


# ---- the mixed coder's cap on the files of a launch: HVC_HUFF_MIXED_MAX_FILES (csrc/hvc_huff_mixed_plan.h) -----------------------
MAX_FILES = 65535
E_TOO_LARGE = -7
SPEC_BYTES = 276             # sizeof(hvc_huff_spec): bits[16], vals[256], n_vals, pad


def coder_records(hvc):
    """(info, D records): 8 x 8 4:4:4, the smallest frame the coder takes -- three planes of one block, three units a file;
    sparse coefficients inside the categories the default tables code"""
    info = hvc.hvc.jpeg_encoder_layout(8, 8, 444, 75)
    assert info.coef_count == 192 and C.sizeof(hvc.hvc.HuffSpec) == SPEC_BYTES
    rng = np.random.default_rng(9900)
    rec = rng.integers(-60, 61, size=(D, 3, 64)) * (rng.random(size=(D, 3, 64)) < 0.25)
    rec[:, :, 0] = rng.integers(-500, 501, size=(D, 3))
    rec[::7, :, 63] = rng.integers(1, 9, size=(len(rec[::7]), 3))              # some blocks without an EOB
    return info, rec.astype(np.int16).reshape(D, 192)


def run_coder(hvc, ctx, info, rec, n, optimised, cap):
    """hvc_huffman_encode_frames_mixed over n frames, frame i = record i % D, device memory -> (return code, the output buffer
    whole (cap offered, GUARD more behind it), offsets [n + 1], status [n], the specs' bytes [n][4][SPEC_BYTES])"""
    import torch
    infos, _ = mc.replicate(hvc.hvc.JpegInfo, [info], n)
    coefs = np.ascontiguousarray(rec[np.arange(n) % D]).reshape(-1)
    status = np.full(n, 77, dtype=np.int32)
    specs = np.full((n, 4, SPEC_BYTES), FILL, dtype=np.uint8)
    d_c, d_out, d_off = to_device(coefs, np.full(cap + GUARD, FILL, dtype=np.uint8), np.full(n + 1, -1, dtype=np.int64))
    r = hvc.lib().hvc_huffman_encode_frames_mixed(
        ctx._h, infos, d_c.data_ptr(), mc.size_array(192 * np.arange(n)), n, hvc.hvc.HVC_HUFF["optimised" if optimised else "default"],
        d_out.data_ptr(), cap, d_off.data_ptr(), (C.c_int * n).from_buffer(status),
        (hvc.hvc.HuffSpec * (4 * n)).from_buffer(specs) if optimised else None, 1)
    ctx.synchronize()
    return r, d_out.cpu().numpy(), d_off.cpu().numpy(), status, specs


@pytest.mark.parametrize("optimised", [False, True], ids=["default", "optimised"])
def test_the_coder_takes_65535_files(hvc, ctx, optimised):
    """every segment and -- optimised: k_huff_build with 65535 rows -- every frame's four tables are the host coder's"""
    from test_gpu_huffman_mixed import host_segment
    info, rec = coder_records(hvc)
    want = [host_segment(info, rec[r], optimised) for r in range(D)]
    assert all(isinstance(w[0], bytes) for w in want)                         # the host coder takes every record
    n = MAX_FILES
    lens = np.array([len(w[0]) for w in want], dtype=np.int64)[np.arange(n) % D]
    offsets = np.concatenate([[0], np.cumsum(lens)])
    total = int(offsets[-1])
    r, out, off, status, specs = run_coder(hvc, ctx, info, rec, n, optimised, total)
    assert r == 0 and (status == 0).all()
    assert np.array_equal(off, offsets)
    whole = b"".join(want[f % D][0] for f in range(n))
    assert out[:total].tobytes() == whole and (out[total:] == FILL).all()
    if optimised:
        exp = np.zeros((D, 4, SPEC_BYTES), dtype=np.uint8)
        for k, (_, tables) in enumerate(want):
            for t, pair in enumerate(tables):
                exp[k, t] = np.frombuffer(bytes(hvc.hvc.HuffSpec.from_pair(*pair)), dtype=np.uint8)
        exp = exp[np.arange(n) % D]
        n_vals = exp[:, :, 272].astype(np.int64) + 256 * exp[:, :, 273].astype(np.int64)
        assert np.array_equal(specs[:, :, :16], exp[:, :, :16])                # bits
        assert np.array_equal(specs[:, :, 272:274], exp[:, :, 272:274])        # n_vals
        used = np.arange(256)[None, None, :] < n_vals[:, :, None]
        assert np.array_equal(specs[:, :, 16:272][used], exp[:, :, 16:272][used])   # vals[:n_vals]
        assert len({w[0] for w in want}) > D // 2 and len({repr(w[1]) for w in want}) > D // 2


def test_the_coder_refuses_the_65536th_file(hvc, ctx):
    """HVC_E_TOO_LARGE from the plan: nothing is launched, the output, the offsets and the status array keep their fill"""
    info, rec = coder_records(hvc)
    for optimised in (False, True):
        r, out, off, status, specs = run_coder(hvc, ctx, info, rec, MAX_FILES + 1, optimised, 1 << 24)
        assert r == E_TOO_LARGE
        assert (out == FILL).all() and (off == -1).all() and (status == 77).all() and (specs == FILL).all()


def test_the_file_pipeline_closes_a_chunk_at_65535_files(hvc, ctx):
    """hvc_jpeg_encode_batch_mixed_gpu over 65537 frames of 8 x 8 4:4:4: the records fill no chunk (24 MB of 64 MiB), the coder's
    cap closes the first at 65535 files; every file is jpeg_encode's of the same frame"""
    n = MAX_FILES + 2
    rng = np.random.default_rng(9950)
    raws = rng.integers(0, 256, size=(D, 192), dtype=np.uint8)
    raws[::2] = rng.integers(100, 140, size=raws[::2].shape, dtype=np.uint8)  # smooth ones: short segments
    quality = [(50, 75, 90)[r % 3] for r in range(D)]
    want = [ctx.jpeg_encode(*orc.split_yuv(raws[r].tobytes(), 8, 8, 444), 8, 8, 444, quality[r]) for r in range(D)]
    room = 2048
    assert max(len(w) for w in want) < room and len(set(want)) == D
    lay = hvc.hvc.EncoderMixedLayout([(8, 8, 444, quality[f % D]) for f in range(n)])
    buf = np.full((n, room), FILL, dtype=np.uint8)
    results = ctx.jpeg_encode_batch_mixed_gpu([raws[f % D] for f in range(n)], layout=lay, threads=8, outs=list(buf), caps=[room] * n)
    st = ctx.last_batch_stats
    assert (st.chunks, st.frames_per_chunk) == (2, MAX_FILES)
    assert sum(ctx.last_mixed_coder_files()) == n
    sizes = np.array([len(w) for w in want])[np.arange(n) % D]
    assert [r[0] for r in results] == [0] * n and [r[2] for r in results] == sizes.tolist()
    expect = np.full((D, room), FILL, dtype=np.uint8)
    for r, w in enumerate(want):
        expect[r, :len(w)] = np.frombuffer(w, dtype=np.uint8)
    assert np.array_equal(buf, expect[np.arange(n) % D])                      # every file, and the fill behind every file


# ---- the mixed reader's cap on the table sets of a chunk: HVC_HDM_MAX_TABLE_SETS (csrc/hvc_mixed_reader.h) ------------------------
_TABLE_SETS = {}


def table_set_case(hvc):
    """(files, the positions past the cap, the host reader's record of every file)"""
    if not _TABLE_SETS:
        files, reusers = mc.table_set_files()
        firsts = [f for k, f in enumerate(files) if k not in reusers]
        assert len({mc.dht_payload(f) for f in firsts}) >= 516                # (520: tests/test_mixed_counts.py)
        beyond = mc.beyond_the_table_sets(files)
        assert len(beyond) == 8 and not set(beyond) & set(reusers)            # the re-users' sets are among the first 512
        _TABLE_SETS["all"] = (files, beyond, [hvc.hvc.jpeg_entropy_decode(f)[1] for f in files])
    return _TABLE_SETS["all"]


def decode_files(hvc, ctx, files, reader, threads):
    ctx.set_mixed_reader(reader)
    lay = hvc.hvc.MixedLayout(files, 8)                    # records of whole blocks on 8 bytes: they touch, no byte is nobody's
    buf = np.full(lay.total_bytes + GUARD, FILL, dtype=np.uint8)
    res = ctx.jpeg_decode_batch_mixed(files, threads=threads, layout=lay, pixels=buf)   # chunk_bytes 0 = 64 MiB: 270 KB of records
    st = ctx.last_batch_stats
    # one chunk holds every file (the cut does not look at the reader).  hvc_batch_stats.chunks adds the chunks of the host
    # reader's pass over the files the GPU reader handed back (decode_batch_mixed_impl's tail): one more chunk here
    assert st.frames_per_chunk == len(files) and st.chunks == (2 if reader == "gpu" else 1)
    return buf, [r[0] for r in res], ctx.last_mixed_reader_files()


@pytest.mark.parametrize("threads", [1, 3])
def test_more_table_sets_than_a_chunk_has_room_for(hvc, ctx, threads):
    """528 files with 520 table sets in one chunk: the files of the sets past the 512th go to the host reader, a file whose set
    is among the 512 is found by the search and stays on the GPU; the bytes are the host reader's run's"""
    files, beyond, _ = table_set_case(hvc)
    want, want_st, (g0, h0) = decode_files(hvc, ctx, files, "host", threads)
    assert want_st == [0] * len(files) and (g0, h0) == (0, len(files))
    assert not (want[:-GUARD] == FILL).all() and (want[-GUARD:] == FILL).all()
    got, got_st, (g, h) = decode_files(hvc, ctx, files, "gpu", threads)
    assert got_st == [0] * len(files)
    assert np.array_equal(got, want)
    assert g + h == len(files) == 528
    if threads == 1:                                        # one worker prepares the files in file order
        assert (g, h) == (len(files) - len(beyond), len(beyond)) == (520, 8)


def test_the_reader_alone_with_more_table_sets_than_it_has_room_for(hvc, ctx):
    """hvc_jpeg_entropy_decode_gpu_mixed prepares the files in file order on the calling thread"""
    files, beyond, records = table_set_case(hvc)
    lay = hvc.hvc.MixedLayout(files, 8)
    total = hvc.hvc.mixed_coef_offsets(lay)[1]
    buf = np.full(total + GUARD, FILL16, dtype=np.int16)
    got = ctx.jpeg_entropy_decode_gpu_mixed(files, layout=lay, coefs=buf)
    assert (buf[total:] == FILL16).all()
    for k, (status, info, rec, used) in enumerate(got):
        assert status == 0 and np.array_equal(rec, records[k]), k
    assert [k for k, g in enumerate(got) if g[3] != 1] == beyond
