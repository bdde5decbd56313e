"""The parametric fixed-point DCT (hvc_dct_*, hvc_dct_fixed.hip) on the CPU: restatements of the model's
Dct.Fixed_point and of the float64 reference (jpeg/model/src/dct.ml:210-218, 443-482), held against the reference's data
(G11, tests/golden/g11_dct_fixed.json) and against the library's host-side tables and generator; the proof over
hvc_dct_spec.h that every stored value fits int32 and every sum int64; the cross-check with the two Hardcaml twins at
(12, 4); and the `dct` command line's arguments."""
import json
import math
import os
import re
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G11 = json.load(open(os.path.join(ROOT, "tests", "golden", "g11_dct_fixed.json")))
SPEC = os.path.join(ROOT, "video-coding_amd", "csrc", "hvc_dct_spec.h")
M = np.array([struct.unpack("<d", struct.pack("<Q", b))[0] for b in G11["matrix_bits"]]).reshape(8, 8)
SEARCH = [(fr, ft, ir, it) for fr in range(8, 17) for ft in range(6) for ir in range(8, 17) for it in range(6)]
MASK64 = (1 << 64) - 1


# ---- restatements ----------------------------------------------------------------------------------------------------
def fixed_coefs(p, m=M):
    """fixed_coefs ~fixed_prec:p m: round_nearest(m * 2^p) (no entry is a tie: test_rom_has_no_ties)"""
    x = np.ldexp(np.asarray(m, dtype=np.float64), p)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def rnd(x, p):
    """round ~fixed_prec:p, ties away from zero, on int64 arrays (p > 0)"""
    x = np.asarray(x, dtype=np.int64)
    h = np.int64(1 << (p - 1))
    return np.where(x < 0, (x - h + ((1 << p) - 1)) >> p, (x + h) >> p)


def round_matrix(x, p):
    if p == 0:
        return np.asarray(x, dtype=np.int64)
    if p < 0:
        return np.asarray(x, dtype=np.int64) << -p
    return rnd(x, p)


def transform(x, rom_prec, tp, inverse=False):
    """Fixed_point.forward_transform / inverse_transform on [..., 8, 8] int arrays"""
    c = fixed_coefs(rom_prec, M.T if inverse else M)
    t = round_matrix(np.matmul(c, np.asarray(x, dtype=np.int64)), rom_prec - tp)
    return round_matrix(np.matmul(t, c.T), rom_prec + tp)


def fmul(a, b):
    """Matrix8x8.fmul in pure Python floats: sum from 0.0, k = 0..7 in order"""
    out = [[0.0] * 8 for _ in range(8)]
    for r in range(8):
        for c in range(8):
            s = 0.0
            for k in range(8):
                s = s + a[r][k] * b[k][c]
            out[r][c] = s
    return out


def reference(x, inverse=False):
    """fmul (fmul F X) F^T, F = M or M^T, one block -> float64 [8, 8]"""
    f = (M.T if inverse else M).tolist()
    ft = [list(r) for r in zip(*f)]
    return np.array(fmul(fmul(f, [[float(v) for v in row] for row in np.asarray(x).tolist()]), ft))


def reference_np(x, inverse=False):
    """the same, vectorised over [..., 8, 8] (numpy multiplies and adds apart: no contraction), same order"""
    f = M.T if inverse else M
    x = np.asarray(x, dtype=np.float64)

    def mul(a, b):
        out = np.zeros(np.broadcast_shapes(a.shape, b.shape))
        for k in range(8):
            out = out + a[..., :, k:k + 1] * b[..., k:k + 1, :]
        return out
    return mul(mul(f, x), f.T)


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def blocks(seed, rng, first, n):
    """hvc_dct_blocks as include/hvc_jpeg.h documents it, in Python integers -> int64 [n, 8, 8]"""
    out = np.zeros((n, 64), dtype=np.int64)
    for b in range(n):
        i = first + b
        for k in range(32):
            u = mix64((seed + 0x9E3779B97F4A7C15 * (32 * i + k + 1)) & MASK64)
            out[b, 2 * k] = (((u & 0xFFFFFFFF) * 2 * rng) >> 32) - rng
            out[b, 2 * k + 1] = (((u >> 32) * 2 * rng) >> 32) - rng
    return out.reshape(n, 8, 8)


def round_trip_errors(x, fr, ft, ir, it):
    """max |x - inverse(forward(x))| per block"""
    y = transform(transform(x, fr, ft), ir, it, inverse=True)
    return np.abs(np.asarray(x, dtype=np.int64) - y).reshape(len(x), 64).max(axis=1)


def worst(errors):
    """(max error, smallest block index with it)"""
    e = np.asarray(errors)
    return e.max(), int(np.argmax(e == e.max()))


# ---- the fixture -----------------------------------------------------------------------------------------------------
def test_restatements_reproduce_the_fixture():
    for i, want in G11["scaling"]:
        assert min(127, max(-128, int(rnd(i, 3)))) == want, i
    assert [M.max(), M.min()] == G11["coef_range"]
    assert M.T.max() == G11["coef_range"][0]
    # the ordered float64 restatement agrees with its vectorised form to the bit
    x = blocks(3, 200, 0, 4)
    for inv in (False, True):
        for b in x:
            assert np.array_equal(reference(b, inv), reference_np(b, inv))


def test_matrix_is_the_static_x86_matrix():
    import video_coding_amd as hvc
    hvc.build()
    got = hvc.dct_matrix()
    assert [struct.unpack("<Q", struct.pack("<d", v))[0] for v in got.reshape(-1)] == G11["matrix_bits"]


def test_rom_is_fixed_coefs_at_every_precision():
    import video_coding_amd as hvc
    for p in range(0, 17):
        assert np.array_equal(hvc.dct_rom(p), fixed_coefs(p)), p
    with pytest.raises(hvc.HvcError) as e:
        hvc.dct_rom(17)
    assert e.value.code == -5


def test_rom_has_no_ties():
    """M * 2^p is never k + 1/2 at an accepted rom_prec, so the tie rule of round_nearest never matters"""
    for p in range(0, 17):
        x = np.abs(np.ldexp(M, p))
        assert not np.any(x - np.floor(x) == 0.5), p


def test_generator_is_the_documented_function():
    import video_coding_amd as hvc
    for seed, rng, first, n in ((0, 128, 0, 5), (7, 1, 3, 4), (2 ** 64 - 1, 2048, 2 ** 40, 3), (12345, 32768, 99, 2)):
        got = hvc.dct_blocks(seed, rng, first, n)
        assert np.array_equal(got, blocks(seed, rng, first, n)), (seed, rng, first)
        assert got.min() >= -rng and got.max() < rng
    # a pure function of (seed, index): a later start sees the same blocks
    assert np.array_equal(hvc.dct_blocks(5, 128, 0, 10)[4:], hvc.dct_blocks(5, 128, 4, 6))
    big = hvc.dct_blocks(1, 128, 0, 2000)
    assert big.min() == -128 and big.max() == 127
    for bad in (0, 32769):
        with pytest.raises(hvc.HvcError):
            hvc.dct_blocks(0, bad, 0, 1)


# ---- the widths of hvc_dct_spec.h --------------------------------------------------------------------------------
def spec_defines():
    d = {}
    for m in re.finditer(r"^#define (HVC_DCT_\w+) (.+?)(?:\s*/\*.*)?$", open(SPEC).read(), re.M):
        d[m.group(1)] = eval(re.sub(r"HVC_DCT_\w+", lambda n: str(d[n.group(0)]), m.group(2).strip()), {})
    return d


def bounds(rom_prec, tp, xmax, inverse):
    """largest |C X| sum, |T|, |T C^T| sum and |Y| over every |x| <= xmax, from the ROM's row absolute sums"""
    c = fixed_coefs(rom_prec, M.T if inverse else M)
    s = [int(v) for v in np.abs(c).sum(axis=1)]
    acc1 = [si * xmax for si in s]
    t = [int(round_matrix(a, rom_prec - tp)) for a in acc1]   # |round(a)| <= round(|a|): round is odd and monotone
    acc2 = max(ti * sj for ti in t for sj in s)
    return max(acc1), max(t), acc2, int(round_matrix(acc2, rom_prec + tp))


def test_every_stored_value_fits_int32_and_every_sum_int64():
    d = spec_defines()
    assert d["HVC_DCT_ACC_BITS"] == 64 and d["HVC_DCT_STORE_BITS"] == 32
    store, acc = 2 ** (d["HVC_DCT_STORE_BITS"] - 1), 2 ** (d["HVC_DCT_ACC_BITS"] - 1)
    fwd_out = 0
    for p in range(d["HVC_DCT_ROM_PREC_MAX"] + 1):
        for tp in range(d["HVC_DCT_TP_MAX"] + 1):
            for inverse, xmax in ((False, d["HVC_DCT_FWD_IN_MAX"]), (True, d["HVC_DCT_INV_IN_MAX"])):
                a1, t, a2, y = bounds(p, tp, xmax, inverse)
                assert xmax < store and t < store and y < store, (p, tp, inverse)
                # a sum of 8 products of int32 operands, each partial sum within the final bound's
                assert a1 < acc and a2 < acc and 8 * store * 2 ** 15 < acc, (p, tp, inverse)
                if not inverse:
                    fwd_out = max(fwd_out, y)
    # the accepted inverse range covers every accepted forward call's output
    assert fwd_out <= d["HVC_DCT_INV_IN_MAX"]
    # ... and the ROM entries are int16, so every product is int32 x int16
    assert max(int(np.abs(fixed_coefs(p)).max()) for p in range(17)) < 2 ** 15


def test_bounds_are_reached_by_sign_patterns():
    """the bound of each output is met by the input whose signs follow its row pair (a sanity check of bounds())"""
    p, tp = 12, 2
    c = fixed_coefs(p)
    x = 2048 * np.sign(np.outer(c[0], c[0]))
    _, t, _, y = bounds(p, tp, 2048, False)
    assert abs(int(transform(x, p, tp)[0, 0])) == y


# ---- the Hardcaml twins at (12, 4) ---------------------------------------------------------------------------------
def test_fixed_point_at_12_4_is_both_twins_before_the_clip():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_hardcaml_encoder_twin import fdct_rtl
    from test_hardcaml_twin import idct_rtl
    rng = np.random.default_rng(11)
    # the encoder twin: level-shifted pixels; no wrap and no saturation for them (hvc_hardcaml_fwd_spec.h's proof)
    x = rng.integers(-128, 128, size=(500, 8, 8))
    _, r = fdct_rtl(x)
    y = transform(x, 12, 4)
    assert np.abs(y).max() <= 2047
    assert np.array_equal(r, y)
    # the decoder twin: 12-bit coefficients small enough that its 19-bit pass 1 does not wrap and the output fits 8 bits
    x = rng.integers(-60, 61, size=(500, 8, 8))
    t, r = idct_rtl(x)
    y = transform(x, 12, 4, inverse=True)
    keep = np.abs(y).reshape(500, -1).max(axis=1) <= 127
    assert keep.sum() > 100
    assert np.array_equal(r[keep], y[keep])


# ---- the command line ----------------------------------------------------------------------------------------------
def test_dct_arguments():
    from video_coding_amd.__main__ import dct_search_configs, parser
    a = parser().parse_args(["dct", "forward"])
    assert (a.rom_prec, a.transpose_prec, a.input_range, a.count, a.seed, a.block) == (12, 2, 200, 1, 0, None)
    a = parser().parse_args(["dct", "inverse", "-rom-prec", "14", "-transpose-prec", "3", "-input-range", "900",
                             "-count", "50", "-seed", "4", "-block", "17"])
    assert (a.dct_cmd, a.rom_prec, a.transpose_prec, a.input_range, a.count, a.seed, a.block) == \
        ("inverse", 14, 3, 900, 50, 4, 17)
    a = parser().parse_args(["dct", "both", "-fwd-rom-prec", "10", "-inv-transpose-prec", "5", "-count", "1000"])
    assert (a.fwd_rom_prec, a.fwd_transpose_prec, a.inv_rom_prec, a.inv_transpose_prec, a.count) == (10, 2, 12, 5, 1000)
    a = parser().parse_args(["dct", "search"])
    assert (a.count, a.seed) == (10000, 0)
    assert dct_search_configs() == SEARCH and len(SEARCH) == 2916
    with pytest.raises(SystemExit):
        parser().parse_args(["dct", "search", "-block", "3"])
