"""The Hardcaml RTL twin (hvc_set_arithmetic HVC_ARITH_HARDCAML), CPU side: a numpy int64 restatement of the RTL
decoder's block datapath held against the reference's RTL vectors (tests/golden/g9_hardcaml.json), and an
interval-arithmetic proof over the constants of video-coding_amd/csrc/hvc_hardcaml_spec.h that the kernel's int32
arithmetic is exact for every input.  tests/test_gpu_hardcaml.py holds the kernel against this restatement."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SPEC = os.path.join(ROOT, "video-coding_amd", "csrc", "hvc_hardcaml_spec.h")

with open(os.path.join(GOLDEN, "g9_hardcaml.json")) as _f:
    G9 = json.load(_f)
with open(os.path.join(GOLDEN, "g2_mouse480_blocks.json")) as _f:
    G2 = json.load(_f)

# jpeg/model/src/zigzag.ml:3-69  inverse[zz] = raster
ZI = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
               14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46,
               53, 60, 61, 54, 47, 55, 62, 63])
ROM = np.array(G9["rom"], dtype=np.int64).reshape(8, 8)


def sext(x, bits):
    x = np.asarray(x, dtype=np.int64) & ((1 << bits) - 1)
    return np.where(x >= 1 << (bits - 1), x - (1 << bits), x)


def rnd(x, p):
    """Hardcaml_fixed_point's tie_away_from_zero by p bits"""
    return (x + (1 << (p - 1)) - (x < 0)) >> p


def idct_rtl(X):
    """Dct.Make(Idct_config) on [..., 8, 8] 12-bit inputs -> (T with 4 fractional bits, R in [-128, 127])"""
    X = np.asarray(X, dtype=np.int64)
    T = sext(rnd(np.matmul(ROM, X), 8), 19)
    R = np.clip(rnd(np.matmul(T, ROM.T), 16), -128, 127)
    return T, R


def dequant_rtl(coefs_zz, q_zz):
    """records [..., 64] int16 in zig-zag order, table [64] (16-bit, zig-zag) -> dequantised [..., 8, 8] natural order"""
    c = sext(coefs_zz, 12)
    d = sext((np.asarray(q_zz, dtype=np.int64) & 0xFF) * c, 12)
    out = np.zeros(d.shape, dtype=np.int64)
    out[..., ZI] = d
    return out.reshape(d.shape[:-1] + (8, 8))


def hardcaml_blocks(coefs_zz, q_zz):
    """steps 1-5 of the RTL: int16 records [..., 64] -> pixels [..., 8, 8] uint8"""
    return (idct_rtl(dequant_rtl(coefs_zz, q_zz))[1] + 128).astype(np.uint8)


def spec_defines():
    """the #defines of hvc_hardcaml_spec.h: integer expressions of other names, or lists of integers"""
    d = {}
    for m in re.finditer(r"^#define (HVC_HC_\w+) (.+?)(?:\s*/\*.*)?$", open(SPEC).read(), re.M):
        name, val = m.group(1), m.group(2).strip()
        if "," in val:
            d[name] = [int(v) for v in val.split(",")]
        else:
            d[name] = eval(re.sub(r"HVC_HC_\w+", lambda n: str(d[n.group(0)]), val), {})
    return d


def test_restatement_reproduces_the_idct_rtl_vector():
    v = G9["idct"]
    T, R = idct_rtl(np.array(v["dct_inputs"]).reshape(8, 8))
    assert T.reshape(-1).tolist() == v["transpose"]
    assert R.reshape(-1).tolist() == v["pixels"]
    assert min(v["pixels"]) == -128 and max(v["pixels"]) == 127   # the vector exercises the saturation


def test_restatement_reproduces_mouse480_rtl_blocks():
    for b, want in zip(G2["blocks"], G9["mouse_blocks"]):
        assert b["block_number"] == want["block_number"]
        coefs = list(b["coefs_lo12"])   # (zig-zag order, low 12 bits; the DC entry is the difference)
        coefs[0] = b["dc_pred_after"]   # the absolute DC the RTL's predictor holds
        dq = sext(np.array(b["dequant_lo12"]), 12).reshape(8, 8)   # natural order
        # the coefficients the fixture's dequantised values came from sit where dequant_rtl places them
        assert np.array_equal(dequant_rtl(np.array(coefs), np.ones(64)) != 0, dq != 0)
        px = (idct_rtl(dq)[1] + 128).reshape(-1)
        assert px.tolist() == want["pixels"], b["block_number"]
        assert int(np.abs(px - np.array(b["recon"])).max()) == want["max_reconstructed_diff"]
    assert [m["max_reconstructed_diff"] for m in G9["mouse_blocks"]] == [1, 1, 1, 1, 0, 0]


def test_rom_from_cos_and_from_the_spec_header():
    # Float.round_nearest (half away from zero) of 4096 * the inverse DCT matrix; the x86 static table differs from cos
    # in the last bits only, which no rounding here can see
    inv = [[math.sqrt((1 if k == 0 else 2) / 8) * math.cos(math.pi / 8 * (n + 0.5) * k) for k in range(8)] for n in range(8)]
    rom = [[int(math.floor(abs(x) * 4096 + 0.5)) * (1 if x >= 0 else -1) for x in row] for row in inv]
    assert rom == ROM.tolist()
    d = spec_defines()
    assert [d["HVC_HC_ROM_R%d" % r] for r in range(8)] == ROM.tolist()
    assert ROM[0].tolist() == [1448, 2009, 1892, 1703, 1448, 1138, 784, 400]


def test_rom_symmetry_the_butterfly_relies_on():
    for r in range(8):
        for k in range(8):
            assert ROM[7 - r][k] == (-1) ** k * ROM[r][k]


def test_int32_bounds_over_the_spec_header():
    """Both passes on intervals, with the constants and shifts the kernel is compiled from.  Every int32 value the kernel
    forms (dot2 partial sums, butterfly sums, the rounding addends, the mul24 / mad24 chains) stays inside int32, pass 1's
    output needs fewer than 19 bits (the RTL's wrap is unreachable), and the mul24 operands fit 24 bits."""
    d = spec_defines()
    C = [d["HVC_HC_ROM_R%d" % r] for r in range(8)]
    I32 = 1 << 31
    qs = d["HVC_HC_QSHIFT"]
    # dequantised operand of pass 1: 16 * sext12(...) as int16
    x_hi = ((1 << (d["HVC_HC_IN_BITS"] - 1)) - 1) << qs
    x_lo = -(1 << (d["HVC_HC_IN_BITS"] - 1)) << qs
    assert -(1 << 15) <= x_lo and x_hi < (1 << 15)
    assert all(-(1 << 15) <= c < (1 << 15) for row in C for c in row)   # dot2 constant halves

    def span(coefs, lo, hi):
        """interval of sum(c * x) for x in [lo, hi]"""
        return (sum(min(c * lo, c * hi) for c in coefs), sum(max(c * lo, c * hi) for c in coefs))

    p1 = d["HVC_HC_P1_SHIFT"]
    t_abs = 0
    for r in range(4):
        for part in ((0, 2), (4, 6), (1, 3), (5, 7), (0, 2, 4, 6), (1, 3, 5, 7)):
            lo, hi = span([C[r][k] for k in part], x_lo, x_hi)
            assert -I32 <= lo and hi < I32
        for sign in (1, -1):
            coefs = [C[r][k] * (sign if k & 1 else 1) for k in range(8)]
            lo, hi = span(coefs, x_lo, x_hi)
            lo, hi = lo - 1, hi + (1 << (p1 - 1))   # RND's addends
            assert -I32 <= lo and hi < I32
            t_abs = max(t_abs, abs(lo >> p1), abs(hi >> p1))
    assert t_abs < 1 << (d["HVC_HC_T_BITS"] - 1), "pass 1's 19-bit wrap reachable"
    assert t_abs < 1 << 23 and all(abs(c) < 1 << 23 for row in C for c in row)   # v_mul_i32_i24 / v_mad_i32_i24
    p2 = d["HVC_HC_P2_SHIFT"]
    add = (1 << (p2 - 1)) + (d["HVC_HC_LEVEL"] << p2)
    for r in range(8):
        for part in ((0, 2, 4, 6), (1, 3, 5, 7), tuple(range(8))):
            lo, hi = span([C[r][k] for k in part], -t_abs, t_abs)
            assert -I32 <= lo - 1 and hi + add < I32


def test_restatement_wraps_coefficients_and_tables_as_the_rtl():
    rng = np.random.default_rng(9)
    c = rng.integers(-32768, 32768, size=(64, 64))
    q = rng.integers(0, 65536, size=64)
    # only the low 12 bits of the coefficient and the low 8 of the table entry reach the datapath
    assert np.array_equal(hardcaml_blocks(c, q), hardcaml_blocks(sext(c, 12), q & 0xFF))
    assert np.array_equal(hardcaml_blocks(c, q), hardcaml_blocks(c + 4096, q + 256))


def test_new_symbols_are_exported_and_cli_parses():
    sys.path.insert(0, ROOT)
    import video_coding_amd as hvc
    L = hvc.lib()
    for s in ("hvc_set_arithmetic", "hvc_get_arithmetic", "hvc_decode_frames_divergence"):
        assert s in hvc.hvc.SYMBOLS and hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "hvc_jpeg.h")).read()
    assert "HVC_ARITH_HARDCAML = 1" in header
    out = subprocess.run([sys.executable, "-m", "video_coding_amd", "simulate", "decoder", "-h"], cwd=ROOT,
                         capture_output=True, text=True)
    assert out.returncode == 0 and "-error-tolerance" in out.stdout and "-blocks" in out.stdout


def test_decode_order_positions_is_mcu_interleaved():
    sys.path.insert(0, ROOT)
    import video_coding_amd as hvc
    info = hvc.hvc.jpeg_read_header(open(os.path.join(GOLDEN, "Mouse480.jpg"), "rb").read())
    pos = hvc.hvc.decode_order_positions(info)
    # 4:2:0 480 x 320: 60 x 40 luma blocks, 30 x 20 per chroma plane; a macroblock is Y0 Y1 Y2 Y3 Cb Cr
    assert pos[:8].tolist() == [0, 1, 60, 61, 2400, 3000, 2, 3]
    assert sorted(pos.tolist()) == list(range(2400 + 600 + 600))
