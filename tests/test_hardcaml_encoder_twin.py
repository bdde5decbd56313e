"""The Hardcaml RTL encoder twin (hvc_set_encode_arithmetic HVC_ARITH_HARDCAML), CPU side: a numpy int64 restatement of
the RTL encoder's forward DCT and quantiser held against the reference's RTL vectors (tests/golden/g10_hardcaml_encoder.json),
a replay of the kernel's schedule against it, and an interval-arithmetic proof over the constants of
video-coding_amd/csrc/hvc_hardcaml_fwd_spec.h that every wrap and saturation of the RTL is unreachable for 8-bit pixels and
that no int32 or i24 operand of the kernel overflows.  tests/test_gpu_hardcaml_encoder.py holds the kernel against this
restatement."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np

from test_hardcaml_twin import G9, ZI, rnd, sext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SPEC = os.path.join(ROOT, "video-coding_amd", "csrc", "hvc_hardcaml_fwd_spec.h")

with open(os.path.join(GOLDEN, "g10_hardcaml_encoder.json")) as _f:
    G10 = json.load(_f)

ROMF = np.array(G10["rom_forward"], dtype=np.int64).reshape(8, 8)
ZF = np.argsort(ZI)   # forward[raster] = zz


def fdct_rtl(X):
    """Dct.Make(Dct_config) on [..., 8, 8] level-shifted 8-bit inputs -> (T with 4 fractional bits, R in [-2048, 2047])"""
    X = np.asarray(X, dtype=np.int64)
    T = sext(rnd(np.matmul(ROMF, X), 8), 15)                              # transpose_bits = 15
    R = np.clip(rnd(sext(np.matmul(T, ROMF.T), 30), 16), -2048, 2047)    # mac_bits = 30, output_bits = 12
    return T, R


def quant_rtl(R, t):
    """quant.ml: the RAM holds 4096 / t (13 bits); q = wrap12(RND(R * (4096 / t), 12))"""
    qr = 4096 // np.asarray(t, dtype=np.int64)
    return sext(rnd(np.asarray(R, dtype=np.int64) * qr, 12), 12)


def hardcaml_encode_blocks(pixels, table_zz):
    """pixels [..., 8, 8] uint8, table [64] in zig-zag order (1..255) -> records [..., 64] int16 in zig-zag order"""
    p = np.asarray(pixels, dtype=np.int64)
    R = fdct_rtl(p - 128)[1].reshape(p.shape[:-2] + (64,))
    t_nat = np.asarray(table_zz, dtype=np.int64)[ZF]   # coefficient k is divided by table[forward[k]]
    return quant_rtl(R, t_nat)[..., ZI].astype(np.int16)


def fixed_quant(d, t):
    """test_quant.ml's fixed_quant"""
    q = 4096 // t
    return (d * q + 2048 - 1) >> 12 if d < 0 else (d * q + 2048) >> 12


def spec_defines():
    d = {}
    for m in re.finditer(r"^#define (HVC_HCE_\w+) (.+?)(?:\s*/\*.*)?$", open(SPEC).read(), re.M):
        name, val = m.group(1), m.group(2).strip()
        if "," in val:
            d[name] = [int(v) for v in val.split(",")]
        else:
            d[name] = eval(re.sub(r"HVC_HCE_\w+", lambda n: str(d[n.group(0)]), val), {})
    return d


def kernel_schedule(pixels, table_zz):
    """the schedule of hvc_hardcaml_fwd_spec.h step by step in int32 / int16 terms (dot2 on int16 pairs, bytes 1-2 of the
    rounded pass-1 sum, the scaled reciprocal and the high half of the quantiser's sum) -> records [n, 64]"""
    d = spec_defines()
    C = np.array([d["HVC_HCE_ROM_R%d" % r] for r in range(8)], dtype=np.int64)
    p = np.asarray(pixels, dtype=np.int64).reshape(-1, 8, 8)
    i16 = lambda v: sext(v, 16)
    i32 = lambda v: sext(v, 32)
    S = [i16(p[:, x] + p[:, 7 - x]) for x in range(4)]   # [n, 8 columns]
    D = [i16(p[:, x] - p[:, 7 - x]) for x in range(4)]
    w = np.zeros((p.shape[0], 8, 8), dtype=np.int64)
    for u in range(8):
        X = D if u & 1 else S
        acc = 0 if u & 1 else -2 * d["HVC_HCE_LEVEL"] * int(C[u][:4].sum())
        v = i32(acc + C[u][0] * X[0] + C[u][1] * X[1])
        v = i32(v + C[u][2] * X[2] + C[u][3] * X[3])
        w[:, u] = i32(v + (1 << (d["HVC_HCE_P1_SHIFT"] - 1)) + (v >> 31))
    T = i16(w >> 8)   # bytes 1-2 of w
    z = np.zeros((p.shape[0], 8, 8), dtype=np.int64)
    qr = ((d["HVC_HCE_QR_NUM"] // np.asarray(table_zz, dtype=np.int64)[ZF]) << d["HVC_HCE_QR_SCALE"]).reshape(8, 8)
    for v_ in range(8):
        E = [i16(T[:, :, y] + T[:, :, 7 - y]) for y in range(4)] if not v_ & 1 else \
            [i16(T[:, :, y] - T[:, :, 7 - y]) for y in range(4)]
        s = i32(C[v_][0] * E[0] + C[v_][1] * E[1])
        s = i32(s + C[v_][2] * E[2] + C[v_][3] * E[3])
        R = i32(s + (1 << (d["HVC_HCE_P2_SHIFT"] - 1)) + (s >> 31)) >> d["HVC_HCE_P2_SHIFT"]
        z[:, :, v_] = i32(R * qr[:, v_] + (1 << (d["HVC_HCE_QZ_SHIFT"] - 1)) + (R >> 31))
    q = i16(z >> 16).reshape(-1, 64)   # the high half
    return q[:, ZI].astype(np.int16)


def test_restatement_reproduces_the_dct_rtl_vector():
    v = G10["dct"]
    T, R = fdct_rtl(np.array(v["dct_inputs"]).reshape(8, 8))
    assert T.reshape(-1).tolist() == v["transpose"]
    assert R.reshape(-1).tolist() == v["pixels"]


def test_rom_three_ways_and_from_the_spec_header():
    # Float.round_nearest (half away from zero) of 4096 * the forward DCT matrix; the x86 static table (which the fixture's
    # generator read) differs from cos in the last bits only, which no rounding here can see
    fwd = [[math.sqrt((1 if u == 0 else 2) / 8) * math.cos(math.pi / 8 * (x + 0.5) * u) for x in range(8)] for u in range(8)]
    rom = [[int(math.floor(abs(f) * 4096 + 0.5)) * (1 if f >= 0 else -1) for f in row] for row in fwd]
    assert rom == ROMF.tolist()
    assert ROMF.tolist() == np.array(G9["rom"]).reshape(8, 8).T.tolist()   # the transpose of the decoder twin's ROM
    d = spec_defines()
    assert [d["HVC_HCE_ROM_R%d" % r] for r in range(8)] == ROMF.tolist()


def test_rom_symmetry_the_butterfly_relies_on():
    for u in range(8):
        for x in range(8):
            assert ROMF[u][7 - x] == (-1) ** u * ROMF[u][x]


def test_quantiser_hand_checked_cases():
    for c in G10["quant_cases"]:
        assert int(quant_rtl(c["d"], c["t"])) == c["expected"] == fixed_quant(c["d"], c["t"])
    assert [(c["d"], c["t"], c["expected"]) for c in G10["quant_cases"]] == [(-188, 2, -94), (709, 1, 709)]


def test_quantiser_equals_fixed_quant_everywhere():
    d = np.arange(-2048, 2048, dtype=np.int64)[:, None]
    t = np.arange(1, 256, dtype=np.int64)[None, :]
    got = quant_rtl(d, t)
    qr = 4096 // t
    want = np.where(d < 0, (d * qr + 2047) >> 12, (d * qr + 2048) >> 12)
    assert np.array_equal(got, want)
    for dd, tt in ((-2048, 1), (2047, 1), (-1, 255), (0, 7), (-188, 2), (1000, 3)):
        assert int(quant_rtl(dd, tt)) == fixed_quant(dd, tt)
    # within 1 of round-to-nearest division (test_quant.ml's test_range bound)
    exact = np.where(d >= 0, np.floor(d / t + 0.5), np.ceil(d / t - 0.5)).astype(np.int64)
    assert np.abs(got - exact).max() <= 1


def test_scaled_reciprocal_rounds_as_the_rtl():
    """the kernel's quantiser (the reciprocal << QR_SCALE, rounding by QZ_SHIFT) equals quant.ml's for every reachable R"""
    d = spec_defines()
    R = np.arange(-2048, 2048, dtype=np.int64)[:, None]
    t = np.arange(1, 256, dtype=np.int64)[None, :]
    qr16 = (d["HVC_HCE_QR_NUM"] // t) << d["HVC_HCE_QR_SCALE"]
    z = R * qr16 + (1 << (d["HVC_HCE_QZ_SHIFT"] - 1)) + (R >> 31)
    assert np.array_equal(z >> d["HVC_HCE_QZ_SHIFT"], quant_rtl(R, t))


def worst_case_blocks():
    """constant 0 and 255, the +-128 patterns matching each ROM row's signs in both directions, impulses at all 64
    positions on 0 and on 255 backgrounds"""
    out = [np.zeros((8, 8)), np.full((8, 8), 255)]
    for u in range(8):
        for v in range(8):
            sgn = np.outer(np.sign(ROMF[u]), np.sign(ROMF[v]))
            out.append(np.where(sgn >= 0, 255, 0))
            out.append(np.where(sgn >= 0, 0, 255))
    for k in range(64):
        a = np.zeros(64)
        a[k] = 255
        out.append(a.reshape(8, 8))
        out.append(255 - a.reshape(8, 8))
    return np.array(out, dtype=np.uint8)


def test_kernel_schedule_equals_the_restatement():
    rng = np.random.default_rng(10)
    px = np.concatenate([worst_case_blocks(), rng.integers(0, 256, (4000, 8, 8)).astype(np.uint8)])
    for tab in (np.ones(64, np.int64), np.array(G10["quant_table"]), np.array(G10["luma95"]), np.full(64, 255),
                rng.integers(1, 256, 64)):
        assert np.array_equal(kernel_schedule(px, tab), hardcaml_encode_blocks(px, tab))


def test_bounds_over_the_spec_header():
    """The schedule on intervals, with the constants and shifts the kernel is compiled from: the RTL's 15-bit transpose
    wrap, 30-bit accumulator, 12-bit saturation and 12-bit quantiser wrap are unreachable; every dot2 operand fits int16,
    every int32 partial sum stays inside int32, and the quantiser's v_mul_i32_i24 operands fit 24 bits."""
    d = spec_defines()
    C = [d["HVC_HCE_ROM_R%d" % r] for r in range(8)]
    I32, I16 = 1 << 31, 1 << 15
    assert all(-I16 <= c < I16 for row in C for c in row)   # dot2 constant halves
    assert d["HVC_HCE_T_BITS"] == 15 and d["HVC_HCE_MAC_BITS"] == 30 and d["HVC_HCE_OUT_BITS"] == 12

    def span(terms, acc=0):
        """interval of acc + sum(c * [lo, hi])"""
        return (acc + sum(min(c * lo, c * hi) for c, (lo, hi) in terms), acc + sum(max(c * lo, c * hi) for c, (lo, hi) in terms))

    pmax = (1 << d["HVC_HCE_IN_BITS"]) - 1
    s_iv, d_iv = (0, 2 * pmax), (-pmax, pmax)   # S and D halves
    assert -I16 <= d_iv[0] and s_iv[1] < I16
    p1 = d["HVC_HCE_P1_SHIFT"]
    t_abs = 0
    for u in range(8):
        iv = d_iv if u & 1 else s_iv
        acc = 0 if u & 1 else -2 * d["HVC_HCE_LEVEL"] * sum(C[u][:4])
        lo, hi = span([(C[u][0], iv), (C[u][1], iv)], acc)
        assert -I32 <= lo and hi < I32
        lo, hi = span([(C[u][k], iv) for k in range(4)], acc)
        lo, hi = lo - 1, hi + (1 << (p1 - 1))   # RND's addends
        assert -I32 <= lo and hi < I32
        t_abs = max(t_abs, abs(lo >> p1), abs(hi >> p1))
    assert t_abs <= 5793   # (|C X| <= 128 * 11 584; the interval also carries RND's addends)
    assert t_abs < 1 << (d["HVC_HCE_T_BITS"] - 1), "pass 1's 15-bit wrap reachable"
    e_iv = (-2 * t_abs, 2 * t_abs)   # E and O halves
    assert -I16 <= e_iv[0] and e_iv[1] < I16
    p2 = d["HVC_HCE_P2_SHIFT"]
    r_abs = 0
    for v in range(8):
        lo, hi = span([(C[v][0], e_iv), (C[v][1], e_iv)])
        assert -I32 <= lo and hi < I32
        lo, hi = span([(C[v][k], e_iv) for k in range(4)])
        assert -(1 << (d["HVC_HCE_MAC_BITS"] - 1)) <= lo and hi < 1 << (d["HVC_HCE_MAC_BITS"] - 1), "30-bit MAC wrap"
        lo, hi = lo - 1, hi + (1 << (p2 - 1))
        assert -I32 <= lo and hi < I32
        r_abs = max(r_abs, abs(lo >> p2), abs(hi >> p2))
    assert r_abs < 1 << (d["HVC_HCE_OUT_BITS"] - 1), "12-bit saturation reachable"
    qr16_max = (d["HVC_HCE_QR_NUM"] // 1) << d["HVC_HCE_QR_SCALE"]
    assert r_abs < 1 << 23 and qr16_max < 1 << 23   # v_mul_i32_i24
    z_hi = r_abs * qr16_max + (1 << (d["HVC_HCE_QZ_SHIFT"] - 1))
    assert z_hi < I32 and -r_abs * qr16_max - 1 >= -I32
    q_abs = max(abs((z_hi) >> d["HVC_HCE_QZ_SHIFT"]), abs((-r_abs * qr16_max - 1 + (1 << 15)) >> d["HVC_HCE_QZ_SHIFT"]))
    assert q_abs < 1 << (d["HVC_HCE_OUT_BITS"] - 1), "the quantiser's 12-bit wrap reachable"


def test_restatement_wraps_nothing_on_8_bit_pixels():
    # the worst cases reach the proved bound exactly and stay inside every width
    T, R = fdct_rtl(worst_case_blocks().astype(np.int64) - 128)
    assert np.abs(T).max() <= 5792 and np.abs(R).max() <= 1024


def test_new_symbols_are_exported_and_cli_parses():
    sys.path.insert(0, ROOT)
    import video_coding_amd as hvc
    L = hvc.lib()
    for s in ("hvc_set_encode_arithmetic", "hvc_get_encode_arithmetic", "hvc_encode_frames_divergence"):
        assert s in hvc.hvc.SYMBOLS and hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "hvc_jpeg.h")).read()
    assert header.count("HVC_ARITH_HARDCAML = 1") == 1   # the encoder reuses the decoder's enum
    assert "hvc_set_encode_arithmetic(hvc_ctx *ctx, int arith)" in header
    out = subprocess.run([sys.executable, "-m", "video_coding_amd", "simulate", "encoder", "-h"], cwd=ROOT,
                         capture_output=True, text=True)
    assert out.returncode == 0 and "-blocks" in out.stdout and "-chroma" in out.stdout and "-out" in out.stdout
    out = subprocess.run([sys.executable, "-m", "video_coding_amd", "model", "encode", "frame", "-h"], cwd=ROOT,
                         capture_output=True, text=True)
    assert out.returncode == 0 and "-arithmetic" in out.stdout
