"""Restart intervals (DRI + RSTn) WRITTEN by the host coder (csrc/hvc_entropy.cpp): hvc_jpeg_header_restart,
hvc_jpeg_entropy_encode_restart, hvc_huffman_optimal_tables_restart and the context setting's refusals.  Host C++ only --
runs without a GPU.  The independent yardstick is tools/jpeg_opt_writer.py (pure Python; restart_interval=, and tables=
for the Annex K tables of tests/golden/g8_code_tables.json); for whole MCU rows the bytes between two markers are also
held against hvc_jpeg_entropy_encode (model-exact) over the sub-frame of those rows, which needs no writer at all."""
import ctypes as C
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden_bytes, golden_json
from helpers import every_symbol_record, jpeg_optimised_tables, synth_pixels
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HVC_OK, HVC_E_INVALID_ARG, HVC_E_RANGE = 0, -1, -5
RST = re.compile(rb"\xff[\xd0-\xd7]")


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    m.build()
    return m.hvc


def annex_k_tables():
    """the default tables as the writer's `tables`: the reference's own printout ([length, code, ...] per symbol), sorted by
    length, then code -> BITS and HUFFVAL"""
    g = golden_json("g8_code_tables.json")
    out = []
    for dc, ac in ((g["dc_luma"], g["ac_luma"]), (g["dc_chroma"], g["ac_chroma"])):
        pair = []
        dcs = [(ln, code, cat) for ln, code, cat in dc if ln]
        acs = [(ln, code, (run << 4) | size) for row in ac for ln, code, run, size in row if ln]
        for syms in (dcs, acs):
            syms = sorted(syms)
            bits = [0] * 17
            for ln, _, _ in syms:
                bits[ln] += 1
            pair.append((bits, [s for _, _, s in syms]))
        out.append(pair)
    return out


def parts(jpg):
    """(header up to and including SOS, DHT bodies, DRI value or None, entropy-coded segment) of a baseline file"""
    i, dht, dri = 2, {}, None
    while True:
        assert jpg[i] == 0xFF
        m = jpg[i + 1]
        n = int.from_bytes(jpg[i + 2:i + 4], "big")
        body = jpg[i + 4:i + 2 + n]
        if m == 0xC4:
            dht[(body[0] >> 4, body[0] & 15)] = bytes(body[1:])
        if m == 0xDD:
            dri = int.from_bytes(body, "big")
        i += 2 + n
        if m == 0xDA:
            break
    assert jpg[-2:] == b"\xff\xd9"
    return bytes(jpg[:i]), dht, dri, bytes(jpg[i:-2])


def writer_accepts(info, w, h, chroma):
    """jpeg_opt_writer's plane geometry (the frame rounded up to whole MCUs) equals the encoder's for this frame"""
    hs, vs = {420: (2, 2), 422: (2, 2), 444: (1, 1)}[chroma]
    Wr, Hr = -(-w // (8 * hs)) * 8 * hs, -(-h // (8 * vs)) * 8 * vs
    for i in range(3):
        c = info.comp[i]
        if (Wr * c.hscale // hs // 8, Hr * c.vscale // vs // 8) != (info.layout[i].blocks_w, info.layout[i].blocks_h):
            return False
    return True


def mcu_grid(info):
    c0 = info.comp[0]
    return c0.decoded_width // (8 * c0.hscale), c0.decoded_height // (8 * c0.vscale)


def frame_record(w, h, chroma, q, seed):
    cw, ch = orc.chroma_dims(chroma, w, h)
    y = synth_pixels(seed, -(-h // 8) * 8, -(-w // 8) * 8)[:h, :w]
    u = synth_pixels(seed + 1, -(-ch // 8) * 8, -(-cw // 8) * 8)[:ch, :cw]
    v = synth_pixels(seed + 2, -(-ch // 8) * 8, -(-cw // 8) * 8)[:ch, :cw]
    default_jpg, coefs = orc.encode_yuv(y, u, v, w, h, chroma, q, want_coefs=True)
    return np.concatenate([c.reshape(-1) for c in coefs]).astype(np.int16), default_jpg


def random_record(sampling, w, h, seed):
    mh, mv = max(s[0] for s in sampling), max(s[1] for s in sampling)
    Wr, Hr = -(-w // (8 * mh)) * 8 * mh, -(-h // (8 * mv)) * 8 * mv
    nblk = sum((Wr * sh // mh // 8) * (Hr * sv // mv // 8) for sh, sv in sampling)
    rng = np.random.Generator(np.random.PCG64(seed))
    blocks = np.zeros((nblk, 64), dtype=np.int16)
    blocks[:, 0] = rng.integers(-900, 901, size=nblk)
    for b in range(nblk):
        k = rng.integers(0, 14)
        blocks[b, rng.choice(np.arange(1, 64), size=k, replace=False)] = rng.integers(-200, 201, size=k)
    return blocks.reshape(-1), (Wr // (8 * mh)) * (Hr // (8 * mv))


QT = np.stack([np.arange(1, 65), np.arange(64, 0, -1)]).astype(np.uint16)


def intervals(info, ri):
    mw, mh = mcu_grid(info)
    return -(-(mw * mh) // ri)


def check_restart_file(hvc, info, rec, w, h, chroma, ri, plain, plain_opt, accepted):
    """both table modes of one record at one interval against the Python writer, the header's layout, the marker sequence
    and the round trip; plain / plain_opt: the files without an interval.  Returns the two files."""
    mw, mh = mcu_grid(info)
    n_mcu = mw * mh
    n_ivl = -(-n_mcu // ri)
    # -- default tables
    jpg = hvc.jpeg_entropy_encode(info, rec, restart_interval=ri)
    hdr, dht, dri, ecs = parts(jpg)
    phdr, pdht, pdri, pecs = parts(plain)
    assert hdr == hvc.jpeg_header(info, restart_interval=ri)
    assert dri == ri and pdri is None and dht == pdht
    # one DRI segment directly in front of SOS, nothing else of the header changes
    sos = phdr.rindex(b"\xff\xda")
    assert hdr == phdr[:sos] + b"\xff\xdd\x00\x04" + ri.to_bytes(2, "big") + phdr[sos:]
    assert [m[1] - 0xD0 for m in RST.findall(ecs)] == [j % 8 for j in range(n_ivl - 1)]
    if ri >= n_mcu:
        assert ecs == pecs  # the DRI segment is written, no marker is, the segment is the plain one
    # -- optimised tables
    specs = hvc.huffman_optimal_tables(info, rec, restart_interval=ri)
    opt = hvc.jpeg_entropy_encode(info, rec, specs, restart_interval=ri)
    assert opt == hvc.jpeg_entropy_encode(info, rec, "optimised", restart_interval=ri)
    ohdr, odht, odri, oecs = parts(opt)
    assert ohdr == hvc.jpeg_header(info, specs, restart_interval=ri) and odri == ri
    for t, (bits, vals) in enumerate(specs):
        assert odht[(t >> 1, t & 1)] == bytes(bits) + bytes(vals)
    assert [m[1] - 0xD0 for m in RST.findall(oecs)] == [j % 8 for j in range(n_ivl - 1)]
    if ri >= n_mcu:
        assert (odht, oecs) == (parts(plain_opt)[1], parts(plain_opt)[3])
    if accepted:
        want = jpeg_optimised_tables(w, h, chroma, info.qtab_array(), rec, table_sets=2, restart_interval=ri)
        _, wdht, wdri, wecs = parts(want)
        assert wdri == ri and oecs == wecs and odht == wdht
        want = jpeg_optimised_tables(w, h, chroma, info.qtab_array(), rec, table_sets=2, restart_interval=ri,
                                     tables=annex_k_tables())
        assert parts(want)[3] == ecs
    # -- both read back to the record with the reader's extension on
    for f in (jpg, opt):
        _, got = hvc.jpeg_entropy_decode(f, restart_markers=True)
        assert np.array_equal(got.reshape(-1)[:rec.size], rec)
    return jpg, opt


def ri_values(info):
    mw, mh = mcu_grid(info)
    n = mw * mh
    return sorted({ri for ri in (1, 2, 3, 7, mw, n - 1, n, n + 5, 65535) if ri >= 1})


# (a 4:2:0 / 4:2:2 frame of width or height 16k + 1 is one the model cannot encode: 19 x 11 there)
GEOMETRIES = [(w, h, chroma) for chroma in (420, 422, 444)
              for (w, h) in ((8, 8), (17, 9) if chroma == 444 else (19, 11), (130, 66), (480, 320))]


def test_the_annex_k_tables_given_to_the_writer_are_the_default_dht_bodies(hvc):
    info = hvc.jpeg_encoder_layout(16, 16, 420, 50)
    _, dht, _, _ = parts(hvc.jpeg_entropy_encode(info, np.zeros(info.coef_count, dtype=np.int16)))
    for ts, pair in enumerate(annex_k_tables()):
        for ac, (bits, vals) in enumerate(pair):
            assert dht[(ac, ts)] == bytes(bits[1:17]) + bytes(vals)


@pytest.mark.parametrize("q", [1, 50, 100])
@pytest.mark.parametrize("w,h,chroma", GEOMETRIES)
def test_restart_file_equals_the_python_writer(hvc, w, h, chroma, q):
    info = hvc.jpeg_encoder_layout(w, h, chroma, q)
    rec, default_jpg = frame_record(w, h, chroma, q, w * 7 + h + q)
    plain = hvc.jpeg_entropy_encode(info, rec)
    assert plain == default_jpg
    plain_opt = hvc.jpeg_entropy_encode(info, rec, "optimised")
    accepted = writer_accepts(info, w, h, chroma)
    for ri in ri_values(info):
        check_restart_file(hvc, info, rec, w, h, chroma, ri, plain, plain_opt, accepted)


def test_the_writer_is_the_yardstick_for_most_geometries(hvc):
    """the comparison with the Python writer above is left out only where its plane geometry differs from the encoder's"""
    accepted = [writer_accepts(hvc.jpeg_encoder_layout(w, h, chroma, 50), w, h, chroma) for w, h, chroma in GEOMETRIES]
    assert sum(accepted) >= len(accepted) * 2 // 3, accepted


def test_mouse480_with_restart_intervals(hvc):
    y, u, v = orc.decode_a_frame(golden_bytes("Mouse480.jpg"))
    default_jpg, coefs = orc.encode_yuv(y, u, v, 480, 320, 420, 75, want_coefs=True)
    rec = np.concatenate([c.reshape(-1) for c in coefs]).astype(np.int16)
    info = hvc.jpeg_encoder_layout(480, 320, 420, 75)
    assert writer_accepts(info, 480, 320, 420)
    plain_opt = hvc.jpeg_entropy_encode(info, rec, "optimised")
    for ri in (1, 30, 599):
        jpg, opt = check_restart_file(hvc, info, rec, 480, 320, 420, ri, default_jpg, plain_opt, True)
        print("Mouse480 q75 Ri %d: %d bytes (plain %d), optimised %d (plain %d)"
              % (ri, len(jpg), len(default_jpg), len(opt), len(plain_opt)))


def test_every_symbol_record_with_restart_intervals(hvc):
    info = hvc.jpeg_encoder_layout(128, 88, 444, 50)
    rec = every_symbol_record(info)
    assert writer_accepts(info, 128, 88, 444)
    plain, plain_opt = hvc.jpeg_entropy_encode(info, rec), hvc.jpeg_entropy_encode(info, rec, "optimised")
    for ri in (1, 5, 16, 175, 176):
        check_restart_file(hvc, info, rec, 128, 88, 444, ri, plain, plain_opt, True)


# -- marker bookkeeping -----------------------------------------------------------------------------------------------

def test_marker_numbers_wrap_and_a_stuffed_ff_stands_in_front_of_a_marker(hvc):
    """200 x 72, Ri = 1, random records: more than 8 intervals (D0 .. D7 wrap) and FF 00 FF Dn -- the pad byte of an
    interval is 0xFF, stuffed, and the marker follows.  The expectation is the Python writer's, and that it CONTAINS such
    places is asserted here, so that the case cannot silently go away."""
    tabs = annex_k_tables()
    for chroma, sampling, want_places in ((420, [(2, 2), (1, 1), (1, 1)], 1), (444, [(1, 1)] * 3, 2)):
        info = hvc.jpeg_encoder_layout(200, 72, chroma, 50)
        assert writer_accepts(info, 200, 72, chroma)
        total = 0
        for seed in range(4):
            rec, n_mcu = random_record(sampling, 200, 72, seed)
            assert rec.size == info.coef_count and n_mcu > 8
            want = jpeg_optimised_tables(200, 72, chroma, QT, rec, table_sets=2, restart_interval=1, tables=tabs)
            wecs = parts(want)[3]
            places = len(re.findall(rb"\xff\x00\xff[\xd0-\xd7]", wecs))
            if seed == 0:
                assert places == want_places
            total += places
            got = hvc.jpeg_entropy_encode(info, rec, restart_interval=1)
            ecs = parts(got)[3]
            assert ecs == wecs
            marks = [m[1] - 0xD0 for m in RST.findall(ecs)]
            assert marks == [j % 8 for j in range(n_mcu - 1)] and len(marks) > 8
            opt = hvc.jpeg_entropy_encode(info, rec, "optimised", restart_interval=1)
            wopt = jpeg_optimised_tables(200, 72, chroma, QT, rec, table_sets=2, restart_interval=1)
            assert parts(opt)[1:] == parts(wopt)[1:]
            for f in (got, opt):
                assert np.array_equal(hvc.jpeg_entropy_decode(f, restart_markers=True)[1].reshape(-1), rec)
        assert total >= want_places


# -- whole MCU rows: the intervals are the sub-frames' segments ------------------------------------------------------------

@pytest.mark.parametrize("chroma", [420, 422, 444])
@pytest.mark.parametrize("w,h", [(480, 320), (128, 96)])
def test_intervals_of_whole_mcu_rows_are_the_sub_frames_segments(hvc, w, h, chroma):
    q = 60
    info = hvc.jpeg_encoder_layout(w, h, chroma, q)
    rec, _ = frame_record(w, h, chroma, q, w + h + chroma)
    mw, mh = mcu_grid(info)
    for k in (1, 2, 3):
        ecs = parts(hvc.jpeg_entropy_encode(info, rec, restart_interval=k * mw))[3]
        pieces = RST.split(ecs)
        assert len(pieces) == -(-mh // k)
        for j, piece in enumerate(pieces):
            r0, r1 = j * k, min(mh, j * k + k)
            sub_h = (r1 - r0) * 8 * info.comp[0].vscale
            sub = hvc.jpeg_encoder_layout(w, sub_h, chroma, q)
            assert mcu_grid(sub) == (mw, r1 - r0)
            cut = []
            for i in range(3):
                L, S, v = info.layout[i], sub.layout[i], info.comp[i].vscale
                assert (S.blocks_w, S.blocks_h) == (L.blocks_w, (r1 - r0) * v)  # no padding blocks of its own
                plane = rec[L.coef_offset:L.coef_offset + L.blocks_w * L.blocks_h * 64].reshape(L.blocks_h, L.blocks_w * 64)
                cut.append(plane[r0 * v:r1 * v].reshape(-1))
            sub_rec = np.concatenate(cut)
            assert sub_rec.size == sub.coef_count
            assert parts(hvc.jpeg_entropy_encode(sub, sub_rec))[3] == piece, (k, j)


# -- round trips through other decoders ----------------------------------------------------------------------------

@pytest.mark.parametrize("chroma", [420, 422, 444])
def test_single_interval_file_decodes_like_the_plain_file(hvc, chroma):
    info = hvc.jpeg_encoder_layout(130, 66, chroma, 50)
    rec, plain = frame_record(130, 66, chroma, 50, 5)
    mw, mh = mcu_grid(info)
    for tables in (None, "optimised"):
        f = hvc.jpeg_entropy_encode(info, rec, tables, restart_interval=mw * mh)
        for a, b in zip(orc.decode_a_frame(f), orc.decode_a_frame(plain)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("chroma", [420, 422, 444])
def test_pil_decodes_restart_files_to_the_plain_files_pixels(hvc, chroma):
    Image = pytest.importorskip("PIL.Image")
    info = hvc.jpeg_encoder_layout(130, 66, chroma, 50)
    rec, plain = frame_record(130, 66, chroma, 50, 9)
    want = np.asarray(Image.open(io.BytesIO(plain)).convert("YCbCr"))
    mw, mh = mcu_grid(info)
    for ri in (1, 3, mw, mw * mh - 1, mw * mh):
        for tables in (None, "optimised"):
            f = hvc.jpeg_entropy_encode(info, rec, tables, restart_interval=ri)
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(f)).convert("YCbCr")), want), (ri, tables)


# -- Ri = 0 ---------------------------------------------------------------------------------------------------------

def raw_encode(hvc, info, specs, ri, rec):
    cap = 8 * rec.size + 8192
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t()
    r = hvc.lib().hvc_jpeg_entropy_encode_restart(C.byref(info), None if specs is None else hvc.huff_specs(specs), ri,
                                                  rec.ctypes.data, out.ctypes.data, cap, C.byref(n))
    return r, out[:n.value].tobytes()


def raw_header(hvc, info, specs, ri):
    out = np.empty(4096, dtype=np.uint8)
    n = C.c_size_t()
    r = hvc.lib().hvc_jpeg_header_restart(C.byref(info), None if specs is None else hvc.huff_specs(specs), ri, out.ctypes.data,
                                          out.size, C.byref(n))
    return r, out[:n.value].tobytes()


def raw_tables(hvc, info, rec, ri):
    out = (hvc.HuffSpec * 4)()
    r = hvc.lib().hvc_huffman_optimal_tables_restart(C.byref(info), rec.ctypes.data, ri, out)
    return r, [s.to_pair() for s in out]


@pytest.mark.parametrize("chroma", [420, 422, 444])
def test_interval_zero_through_the_new_functions_gives_the_old_bytes(hvc, chroma):
    info = hvc.jpeg_encoder_layout(130, 66, chroma, 50)
    rec, plain = frame_record(130, 66, chroma, 50, 3)
    specs = hvc.huffman_optimal_tables(info, rec)
    assert raw_tables(hvc, info, rec, 0) == (HVC_OK, specs)
    assert raw_encode(hvc, info, None, 0, rec) == (HVC_OK, plain)
    assert raw_encode(hvc, info, specs, 0, rec) == (HVC_OK, hvc.jpeg_entropy_encode(info, rec, specs))
    assert raw_header(hvc, info, None, 0) == (HVC_OK, hvc.jpeg_header(info))
    assert raw_header(hvc, info, specs, 0) == (HVC_OK, hvc.jpeg_header(info, specs))


# -- refusals -------------------------------------------------------------------------------------------------------

def test_refusals(hvc):
    L = hvc.lib()
    info = hvc.jpeg_encoder_layout(32, 16, 444, 50)
    rec = np.zeros(info.coef_count, dtype=np.int16)
    for ri in (-1, 65536, 1 << 20):
        assert raw_encode(hvc, info, None, ri, rec)[0] == HVC_E_INVALID_ARG
        assert raw_header(hvc, info, None, ri)[0] == HVC_E_INVALID_ARG
        assert raw_tables(hvc, info, rec, ri)[0] == HVC_E_INVALID_ARG
    n = C.c_size_t()
    out = np.empty(65536, dtype=np.uint8)
    specs = (hvc.HuffSpec * 4)()
    specs[0].bits[0] = 3  # three codes of one bit, no symbol: malformed
    assert L.hvc_jpeg_entropy_encode_restart(None, None, 1, rec.ctypes.data, out.ctypes.data, out.size, C.byref(n)) == HVC_E_INVALID_ARG
    assert L.hvc_jpeg_entropy_encode_restart(C.byref(info), None, 1, None, out.ctypes.data, out.size, C.byref(n)) == HVC_E_INVALID_ARG
    assert L.hvc_jpeg_entropy_encode_restart(C.byref(info), None, 1, rec.ctypes.data, out.ctypes.data, out.size, None) == HVC_E_INVALID_ARG
    assert L.hvc_jpeg_entropy_encode_restart(C.byref(info), None, 1, rec.ctypes.data, out.ctypes.data, 10, C.byref(n)) == HVC_E_INVALID_ARG
    assert L.hvc_jpeg_entropy_encode_restart(C.byref(info), specs, 1, rec.ctypes.data, out.ctypes.data, out.size, C.byref(n)) == HVC_E_INVALID_ARG  # a malformed spec
    assert L.hvc_jpeg_header_restart(None, None, 1, out.ctypes.data, out.size, C.byref(n)) == HVC_E_INVALID_ARG
    assert L.hvc_jpeg_header_restart(C.byref(info), None, 1, out.ctypes.data, out.size, None) == HVC_E_INVALID_ARG
    assert L.hvc_jpeg_header_restart(C.byref(info), None, 1, out.ctypes.data, 10, C.byref(n)) == HVC_E_INVALID_ARG
    assert L.hvc_jpeg_header_restart(C.byref(info), specs, 1, out.ctypes.data, out.size, C.byref(n)) == HVC_E_INVALID_ARG
    assert L.hvc_huffman_optimal_tables_restart(None, rec.ctypes.data, 1, specs) == HVC_E_INVALID_ARG
    assert L.hvc_huffman_optimal_tables_restart(C.byref(info), None, 1, specs) == HVC_E_INVALID_ARG
    assert L.hvc_huffman_optimal_tables_restart(C.byref(info), rec.ctypes.data, 1, None) == HVC_E_INVALID_ARG
    # the context's functions without a context (no GPU needed to be refused)
    v = C.c_int(7)
    assert L.hvc_set_restart_interval(None, 1) == HVC_E_INVALID_ARG
    assert L.hvc_get_restart_interval(None, C.byref(v)) == HVC_E_INVALID_ARG and v.value == 7
    assert L.hvc_huffman_encode_frames_restart(None, C.byref(info), rec.ctypes.data, info.coef_count, 1, 1, 0, out.ctypes.data,
                                               out.size, None, None, 0) == HVC_E_INVALID_ARG


def test_a_dc_difference_of_category_12_can_vanish_or_arise_at_a_reset(hvc):
    info = hvc.jpeg_encoder_layout(16, 8, 444, 50)  # two MCUs of one block per component
    assert mcu_grid(info) == (2, 1)
    rec = np.zeros(info.coef_count, dtype=np.int16).reshape(3, 2, 64)
    # vanishes: 2047 then -2047 is a difference of category 12 in a plain scan; from zero each is category 11
    rec[:, 0, 0], rec[:, 1, 0] = 2047, -2047
    flat = rec.reshape(-1)
    assert raw_encode(hvc, info, None, 0, flat)[0] == HVC_E_RANGE
    assert raw_tables(hvc, info, flat, 0)[0] == HVC_E_RANGE
    r, f = raw_encode(hvc, info, None, 1, flat)
    assert r == HVC_OK and np.array_equal(hvc.jpeg_entropy_decode(f, restart_markers=True)[1].reshape(-1), flat)
    assert raw_tables(hvc, info, flat, 1)[0] == HVC_OK
    assert raw_encode(hvc, info, None, 2, flat)[0] == HVC_E_RANGE  # one interval: the plain scan
    # arises: 1000 then 2500 is a difference of category 11; 2500 from zero is category 12
    rec[:, 0, 0], rec[:, 1, 0] = 1000, 2500
    flat = rec.reshape(-1)
    assert raw_encode(hvc, info, None, 0, flat)[0] == HVC_OK
    assert raw_tables(hvc, info, flat, 0)[0] == HVC_OK
    assert raw_encode(hvc, info, None, 1, flat)[0] == HVC_E_RANGE
    assert raw_tables(hvc, info, flat, 1)[0] == HVC_E_RANGE
    assert raw_encode(hvc, info, hvc.huffman_optimal_tables(info, flat), 1, flat)[0] == HVC_E_RANGE


# -- binding ----------------------------------------------------------------------------------------------------------

NEW = ("hvc_set_restart_interval", "hvc_get_restart_interval", "hvc_jpeg_header_restart", "hvc_jpeg_entropy_encode_restart",
       "hvc_huffman_optimal_tables_restart", "hvc_huffman_encode_frames_restart")


def test_symbols_are_listed_and_exported(hvc):
    for name in NEW:
        assert name in hvc.SYMBOLS and hasattr(hvc.lib(), name), name
    header = open(os.path.join(ROOT, "include", "hvc_jpeg.h")).read()
    for name in NEW:
        assert re.search(r"HVC_API int %s\(" % name, header), name


def test_ocaml_binding_covers_the_new_functions():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_ocaml_binding.py"), "--list-unbound"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ml = open(os.path.join(ROOT, "integration", "ocaml", "hvc.ml")).read()
    for name in NEW:
        assert 'foreign "%s"' % name in ml or 'foreign\n    "%s"' % name in ml, name


def test_capacities_of_the_binding_cover_the_markers(hvc):
    """256 MCUs of nothing but EOBs (14 bits each with the default tables: two bytes with the pad bits): the markers weigh
    as much as the data; the binding's default capacities hold"""
    info = hvc.jpeg_encoder_layout(2048, 8, 444, 50)
    rec = np.zeros(info.coef_count, dtype=np.int16)
    f = hvc.jpeg_entropy_encode(info, rec, restart_interval=1)
    assert len(parts(f)[3]) == 256 * 2 + 255 * 2
    assert hvc.restart_slack(info, 1) == 3 * 256 + 6 and hvc.restart_slack(info, 0) == 0
