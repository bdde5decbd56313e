"""The int path of k_islow (video-coding_amd/csrc/hvc_libjpeg.hip) cannot overflow for a block that passes the guard of
hvc_islow_spec.h, and the operation list of that header is the definition's step.  CPU only.

The guard is  S = SUM |d[k]| <= HVC_IS_GUARD_SUM.  Inside one step every value is an exact integer combination of the
step's eight inputs; the list is replayed on weight vectors, so each operation's weights are known exactly.
  pass 1   column c's inputs have SUM |d| = S_c, SUM S_c = S: a value with weights k is within max |k| * S_c <= max |k| * S,
           and a workspace entry within (A * S_c + 2^10) / 2^11, A = the largest weight of any result
  pass 2   a row's inputs are one workspace entry per column: a value with weights k is within
           SUM |k[c]| (A * S_c / 2^11 + 1/2) <= max |k| * A * S / 2^11 + SUM |k| / 2
Evaluated at S = the guard for every operation: no int32 value wraps (the adds of the rounding terms and of the level
shift included), every multiplicand fits the 24 signed bits of v_mul_i32_i24, every d[k] fits int16.  The bounds ignore
signs, so they are conservative.  Constants, guard and list are read from the header, not restated here."""
import os
import re
import sys
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import libjpeg_reference as lj  # noqa: E402

I32_MAX, I24_MAX, I16_MAX = (1 << 31) - 1, (1 << 23) - 1, (1 << 15) - 1


def spec():
    """({name: int}, [(op, [args])]) of hvc_islow_spec.h"""
    text = open(lj.SPEC).read()
    k = lj.spec_constants()
    body = re.search(r"#define HVC_ISLOW_STEP\(MUL, ADD, SUB, SHL, OUTADD, OUTSUB\)(.*?)\n\n", text, flags=re.S).group(1)
    ops = [(op, [a.strip() for a in args.split(",")]) for op, args in re.findall(r"\b(MUL|ADD|SUB|SHL|OUTADD|OUTSUB)\(([^()]*)\)", body)]
    return k, ops


K, OPS = spec()


def const(k, name):
    neg = name.startswith("-")
    v = k[name.lstrip("-")] if not name.lstrip("-").isdigit() else int(name.lstrip("-"))
    return -v if neg else v


def replay(inputs, on_op=None):
    """the list on `inputs` (8 values with + - * by int); returns the 8 undescaled results.  on_op(op, result, operand)"""
    env = {"v%d" % i: inputs[i] for i in range(8)}
    out = [None] * 8
    for op, a in OPS:
        if op == "MUL":
            r, operand = env[a[1]] * const(K, a[2]), env[a[1]]
        elif op == "SHL":
            r, operand = env[a[1]] * (1 << const(K, a[2])), None
        elif op in ("ADD", "OUTADD"):
            r, operand = env[a[1]] + env[a[2]], None
        else:
            r, operand = env[a[1]] - env[a[2]], None
        if op.startswith("OUT"):
            out[int(a[0])] = r
        else:
            env[a[0]] = r
        if on_op:
            on_op(op, a, r, operand)
    assert all(o is not None for o in out)
    return out


def unit(i):
    v = np.zeros(8, dtype=object)
    v[i] = 1
    return v


def test_the_list_is_the_definitions_step():
    """blocks through the header's list (Python integers) = tools/libjpeg_reference.py, which is held against libjpeg"""
    rng = np.random.default_rng(5)
    c = rng.integers(-300, 301, size=(40, 64)).astype(np.int16)
    c[:20] *= rng.random(size=(20, 64)) < 0.2
    q = rng.integers(1, 256, size=64).astype(np.uint16)
    d = lj.dequantised(c, q).astype(object)
    ws = [[lj.D(o, K["HVC_IS_PASS1_SHIFT"]) for o in replay([d[:, r, col] for r in range(8)])] for col in range(8)]   # ws[col][row]
    px = [[lj.D(o, K["HVC_IS_PASS2_SHIFT"]) + K["HVC_IS_LEVEL"] for o in replay([ws[col][r] for col in range(8)])] for r in range(8)]
    got = np.clip(np.array(px, dtype=np.int64).transpose(2, 0, 1), 0, 255).astype(np.uint8)
    assert np.array_equal(got, lj.islow_blocks(c, q))


class Proof:
    def __init__(self, s):
        self.s, self.checked, self.worst = F(s), 0, {}
        self.a = max(int(np.abs(o).max()) for o in replay([unit(i) for i in range(8)]))  # the largest weight of a result

    def bound(self, w, p):
        w = np.abs(np.asarray(w, dtype=object))
        if p == 1:
            return int(w.max()) * self.s
        return int(w.max()) * self.a * self.s / (1 << K["HVC_IS_PASS1_SHIFT"]) + F(int(w.sum()), 2)

    def fits(self, b, most, what):
        assert b <= most, "%s can reach %s" % (what, float(b))
        self.checked += 1
        self.worst[most] = max(self.worst.get(most, (0, "")), (b / most, what))

    def run(self, p):
        def on_op(op, a, r, operand):
            what = "pass %d %s(%s)" % (p, op, ", ".join(a))
            if operand is not None:
                self.fits(self.bound(operand, p), I24_MAX, "multiplicand of " + what)
            if op.startswith("OUT"):
                sh = K["HVC_IS_PASS%d_SHIFT" % p]
                extra = (1 << (sh - 1)) + (K["HVC_IS_LEVEL"] << sh if p == 2 else 0)  # rounding (+ the level shift in the pack's addend)
                self.fits(self.bound(r, p) + extra, I32_MAX, what + " + rounding")
            else:
                self.fits(self.bound(r, p), I32_MAX, what)
        replay([unit(i) for i in range(8)], on_op)


def test_no_int32_intermediate_overflows_under_the_guard():
    P = Proof(K["HVC_IS_GUARD_SUM"])
    P.fits(P.s, I16_MAX, "a dequantised coefficient (v_pk_mul_lo_u16)")
    P.run(1)
    P.fits(P.bound(unit(0), 2), I24_MAX, "a workspace entry")
    P.run(2)
    assert P.checked > 100
    # what the header says gives way first
    frac, what = P.worst[I32_MAX]
    assert "q2" in what and what.startswith("pass 2"), what
    assert frac > F(9, 10)  # the guard is not needlessly narrow: the tightest bound is within 10 % of int32


def test_the_proof_catches_a_guard_that_is_too_wide():
    P = Proof(K["HVC_IS_GUARD_SUM"] * 5 // 4)
    with pytest.raises(AssertionError):
        P.run(2)


def test_ordinary_blocks_are_far_inside():
    """a DC of 8 * 1023 beside AC terms of a few thousand"""
    assert 8 * 1023 + 5000 <= K["HVC_IS_GUARD_SUM"]


def block(dc, ac, q=1):
    c = np.zeros(64, dtype=np.int64)
    c[0] = dc
    c[lj.ZF[8 * 7 + 7]] = -ac
    return c, np.full(64, q, dtype=np.int64)


def test_classification_at_the_guard_and_one_past_it():
    g = K["HVC_IS_GUARD_SUM"]
    for dc in (0, 1, 1000, 8184, g):
        assert lj.takes_int32_path(*block(dc, g - dc))
        assert lj.takes_int32_path(*block(-dc, g - dc))
        assert not lj.takes_int32_path(*block(dc, g - dc + 1))
    assert lj.takes_int32_path(*block(g // 3, 0, 3)) and not lj.takes_int32_path(*block(g // 3 + 1, 0, 3))
    # every position counts
    c = np.zeros(64, dtype=np.int64)
    c[:] = g // 64
    assert lj.takes_int32_path(c, np.ones(64, dtype=np.int64))
    c[37] += g % 64 + 1
    assert not lj.takes_int32_path(c, np.ones(64, dtype=np.int64))
    # the extremes of the formats: an int16 coefficient times a 16-bit entry
    c, q = block(-32768, 32767)
    assert not lj.takes_int32_path(c, q * 65535)
