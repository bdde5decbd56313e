"""The int32 path of k_decode_scaled (video-coding_amd/csrc/hvc_scaled.hip) cannot overflow for a block that passes the
guard of hvc_scaled_spec.h.  CPU only.

The guard is  WD * DC + WA * AC <= LIMIT  with DC = |d[0]| and AC = the largest |d[k]| of the other positions the
definition reads.  Every value of both passes is bounded in magnitude by a linear form  a * DC + b * AC + c  with
non-negative rational coefficients (the sums of the absolute constants; D(x, n) is at most (|x| + 2^(n-1)) / 2^n in
magnitude).  A linear form over the guard's triangle {DC, AC >= 0, WD * DC + WA * AC <= LIMIT} is largest at one of its three
corners, so evaluating every form there proves the claim for every block inside: no int32 value wraps, and every
multiplicand fits the 24 signed bits of v_mul_i32_i24.  The forms ignore correlations, so the bound is conservative.
The constants and the guard are read from the header, not restated here."""
import os
import sys
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scaled_reference as sr  # noqa: E402

K = sr.spec_constants()
I32_MAX, I24_MAX = (1 << 31) - 1, (1 << 23) - 1


class Form:
    """|value| <= a * DC + b * AC + c"""

    def __init__(self, a=0, b=0, c=0):
        self.a, self.b, self.c = F(a), F(b), F(c)

    def __add__(self, o):  # |x + y|, |x - y| <= |x| + |y|
        return Form(self.a + o.a, self.b + o.b, self.c + o.c)

    def times(self, k):
        k = abs(k)
        return Form(self.a * k, self.b * k, self.c * k)

    def descaled(self, n):
        return Form(self.a / (1 << n), self.b / (1 << n), (self.c + (1 << (n - 1))) / (1 << n))

    def at(self, dc, ac):
        return self.a * dc + self.b * ac + self.c


class Proof:
    def __init__(self, n):
        p = "HVC_S%d_GUARD_" % n
        self.wd, self.wa, self.limit = K[p + "WD"], K[p + "WA"], K[p + "LIMIT"]
        self.corners = [(F(0), F(0)), (F(self.limit, self.wd), F(0)), (F(0), F(self.limit, self.wa))]
        self.checked = 0

    def fits(self, form, most, what):
        for dc, ac in self.corners:
            assert form.at(dc, ac) <= most, "%s can reach %s at DC = %s, AC = %s" % (what, float(form.at(dc, ac)), float(dc), float(ac))
        self.checked += 1

    def mul(self, k, form, what):
        assert abs(k) <= I24_MAX
        self.fits(form, I24_MAX, "multiplicand of " + what)
        out = form.times(k)
        self.fits(out, I32_MAX, what)
        return out

    def total(self, terms, what):
        """a sum or difference of terms, in any order: every partial sum is within the sum of the magnitudes"""
        out = Form()
        for t in terms:
            out = out + t
        self.fits(out, I32_MAX, what)
        return out

    def descale(self, form, n, what):
        self.fits(form + Form(c=1 << (n - 1)), I32_MAX, what + " + rounding")
        return form.descaled(n)


def step4(P, v, sh, what):
    t0 = v[0].times(1 << K["HVC_S4_V0_SHIFT"])
    P.fits(t0, I32_MAX, what + " t0")
    t2 = P.total([P.mul(K["HVC_S4_V2"], v[2], what + " t2"), P.mul(K["HVC_S4_V6"], v[6], what + " t2")], what + " t2")
    te = P.total([t0, t2], what + " t10 / t12")
    o0 = P.total([P.mul(K["HVC_S4_O0_V%d" % i], v[i], what + " o0") for i in (7, 5, 3, 1)], what + " o0")
    o2 = P.total([P.mul(K["HVC_S4_O2_V%d" % i], v[i], what + " o2") for i in (7, 5, 3, 1)], what + " o2")
    r0, r2 = (P.descale(P.total([te, o], what + " result"), sh, what) for o in (o0, o2))
    return Form(max(r0.a, r2.a), max(r0.b, r2.b), max(r0.c, r2.c))  # bounds all four results


def step2(P, v, sh, what):
    t10 = v[0].times(1 << K["HVC_S2_V0_SHIFT"])
    P.fits(t10, I32_MAX, what + " t10")
    t0 = P.total([P.mul(K["HVC_S2_V%d" % i], v[i], what + " t0") for i in (7, 5, 3, 1)], what + " t0")
    return P.descale(P.total([t10, t0], what + " result"), sh, what)


@pytest.mark.parametrize("n", [4, 2])
def test_no_int32_intermediate_overflows_under_the_guard(n):
    P = Proof(n)
    step = step4 if n == 4 else step2
    sh1, sh2 = K["HVC_S%d_PASS1_SHIFT" % n], K["HVC_S%d_PASS2_SHIFT" % n]
    DC, AC = Form(a=1), Form(b=1)
    # pass 1: column 0 has d[0] on top, every other element of every used column is an AC term
    col0 = step(P, [DC] + [AC] * 7, sh1, "pass 1, column 0")
    colc = step(P, [AC] * 8, sh1, "pass 1, other columns")
    # pass 2: a row of the workspace: column 0's result first, the other columns' behind it
    out = step(P, [col0] + [colc] * 7, sh2, "pass 2")
    P.fits(out + Form(c=128), I32_MAX, "sample + 128")
    assert P.checked > 20
    # the crude bound of equal DC and AC terms (1448 / 2391) lies inside the guard, one more does not have to
    m = {4: 1448, 2: 2391}[n]
    assert P.wd * m + P.wa * m <= P.limit


def test_the_proof_catches_a_guard_that_is_too_wide():
    P = Proof(4)
    P.corners = [(dc * 2, ac * 2) for dc, ac in P.corners]
    with pytest.raises(AssertionError):
        step4(P, [step4(P, [Form(a=1)] + [Form(b=1)] * 7, 12, "pass 1")] * 8, 19, "pass 2")


def block(n, dc, ac):
    """one block (unit table) with d[0] = dc and the largest other used term = ac, at the last used position"""
    c = np.zeros(64, dtype=np.int64)
    c[0] = dc
    c[sr.ZF[8 * 7 + 7]] = -ac
    return c, np.ones(64, dtype=np.int64)


@pytest.mark.parametrize("n", [4, 2])
def test_classification_at_the_guard_and_one_past_it(n):
    p = "HVC_S%d_GUARD_" % n
    wd, wa, limit = K[p + "WD"], K[p + "WA"], K[p + "LIMIT"]
    for dc in (0, 1, 1000, 8192, limit // wd):
        ac = (limit - wd * dc) // wa   # the largest AC term the guard admits beside this DC
        assert sr.takes_int32_path(*block(n, dc, ac), n)
        assert sr.takes_int32_path(*block(n, -dc, ac), n)
        assert not sr.takes_int32_path(*block(n, dc, ac + 1), n)
    assert not sr.takes_int32_path(*block(n, limit // wd + 1, 0), n)
    # positions the definition does not read do not count: natural row 4 / column 4 (N = 4), the even ones (N = 2)
    c, q = block(n, 0, 0)
    c[sr.ZF[8 * 4 + 4]] = 32767
    assert sr.takes_int32_path(c, q, n)
    # N = 1 has no guard
    assert sr.takes_int32_path(*block(1, 32767, 32767), 1)
    # the extremes of the formats: an int16 coefficient times a 16-bit entry
    c, q = block(n, 32767, 32767)
    assert not sr.takes_int32_path(c, q * 65535, n)
