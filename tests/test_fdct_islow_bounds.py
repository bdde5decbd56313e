"""The forward DCT of k_fdct_islow (video-coding_amd/csrc/hvc_fdct_islow_dev.h) cannot overflow for 8-bit samples, every
multiplicand fits the 24 signed bits of v_mul_i32_i24, and the quantiser sees no |t| above HVC_FI_T_MAX.  CPU only.

The operation list of hvc_fdct_islow_spec.h is replayed on weight vectors (tools/libjpeg_encode_reference.py parses the
header: the list proved here is the list the kernel expands and the numpy definition replays).  Inside one step every value
is an exact integer combination of the step's eight inputs, so with every input within m its magnitude is at most
SUM |weight| * m, and that bound is reached up to the asymmetry of the two's-complement range.
  pass 1   the inputs are p - LEVEL, p in 0..255: m = LEVEL.  Result i is within B1[i] after its scaling (<< 2, or D(., 11))
  pass 2   column c's eight inputs are result c of the eight rows: m = B1[c]; every bound is taken over the worst column
A bound ignores that the eight inputs of a pass-2 column are not independent of each other: conservative, not exact."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import libjpeg_encode_reference as ler  # noqa: E402

I32_MAX, I24_MAX, I16_MAX = (1 << 31) - 1, (1 << 23) - 1, (1 << 15) - 1
K, OPS = ler.spec_constants(), ler.spec_step()


def unit(i):
    v = np.zeros(8, dtype=object)
    v[i] = 1
    return v


def forms():
    """{name or result index: weights} of the step"""
    return ler.replay_step([unit(i) for i in range(8)], lambda a, k: a * k, lambda a, b: a + b, lambda a, b: a - b, OPS)


def sup(w, m):
    return int(np.abs(np.asarray(w, dtype=object)).sum()) * m


class Proof:
    def __init__(self, level):
        self.f, self.level, self.checked, self.largest_factor = forms(), level, 0, 0

    def fits(self, b, most, what):
        assert b <= most, "%s can reach %d" % (what, b)
        self.checked += 1

    def run(self, m, lo_scale, hi_shift, what):
        """one pass with every input within m -> the bound of each of the eight results after scaling"""
        for op in OPS:
            if op[0] == "MUL":
                self.fits(sup(self.f[op[2]], m), I24_MAX, "%s: the multiplicand of %s" % (what, op[1]))
                self.largest_factor = max(self.largest_factor, abs(op[3]))
            if op[0] in ("MUL", "ADD", "SUB"):
                self.fits(sup(self.f[op[1]], m), I32_MAX, "%s: %s" % (what, op[1]))
        out = []
        for i in range(8):
            kind, w = self.f[i]
            b = sup(w, m)
            if kind == "OUTLO":
                out.append(lo_scale(b))
            else:
                self.fits(b + (1 << (hi_shift - 1)), I32_MAX, "%s: result %d + rounding" % (what, i))
                out.append((b + (1 << (hi_shift - 1))) >> hi_shift)
            self.fits(out[-1], I32_MAX, "%s: result %d" % (what, i))
        return out

    def both(self):
        lo_shl, lo_shr = K["HVC_FI_PASS1_LO_SHL"], K["HVC_FI_PASS2_LO_SHIFT"]
        b1 = self.run(self.level, lambda b: b << lo_shl, K["HVC_FI_PASS1_HI_SHIFT"], "pass 1")
        b2 = self.run(max(b1), lambda b: (b + (1 << (lo_shr - 1))) >> lo_shr, K["HVC_FI_PASS2_HI_SHIFT"], "pass 2")
        return b1, b2


def test_no_value_overflows_and_every_multiplicand_fits_24_bits():
    P = Proof(K["HVC_FI_LEVEL"])
    b1, b2 = P.both()
    assert P.checked > 100
    assert P.largest_factor < 1 << 15, "every constant of the list is below 2^15"
    assert max(b1) <= I16_MAX  # (pass 1's results would even fit int16)
    t_max = max(b2)
    assert t_max == K["HVC_FI_T_MAX"], "hvc_fdct_islow_spec.h states T_MAX = %d, the proof gives %d" % (K["HVC_FI_T_MAX"], t_max)
    # the quantiser: numerator |t| + 4 q in uint32, quotient in int16, for every divisor 8 q, q in 1 .. Q_MAX
    assert t_max + 4 * K["HVC_FI_Q_MAX"] < 1 << 24
    assert (t_max + 4) // 8 <= I16_MAX


def test_the_proof_catches_inputs_that_are_too_wide():
    """16-bit samples would overflow the multiplies of pass 2"""
    with pytest.raises(AssertionError):
        Proof(1 << 15).both()


def test_the_bound_is_not_idle():
    """blocks that come near it: all 0 (the largest DC), and the sign patterns of each basis function"""
    k = np.arange(8)
    basis = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)  # [u][x]
    worst = 0
    for u in range(8):
        for v in range(8):
            s = np.sign(np.outer(basis[u], basis[v]))
            for blk in (np.where(s > 0, 255, 0), np.where(s > 0, 0, 255)):
                worst = max(worst, int(np.abs(ler.fdct_islow(blk.astype(np.uint8))).max()))
    assert worst <= K["HVC_FI_T_MAX"]
    assert worst >= 8192, worst           # all 0: DC = -64 * 128
    assert worst * 2 > K["HVC_FI_T_MAX"]  # the interval bound is within a factor of two of a block that exists


def test_the_list_is_jfdctint():
    """the header's list against jfdctint.c written out by hand (floating DCT within the fixed-point error)"""
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, size=(50, 8, 8)).astype(np.uint8)
    t = ler.fdct_islow(x)
    k = np.arange(8)
    c = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))[:, None]
    want = 8 * np.einsum("ur,brc,vc->buv", c, x.astype(np.float64) - 128, c)
    assert np.abs(t - want).max() < 2.0
