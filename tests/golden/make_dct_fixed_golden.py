#!/usr/bin/env python3
"""Extract the data the parametric fixed-point DCT (hvc_dct_*) is checked against (G11) from the reference's model
and its tests.  CPU only; run once where the reference exists:

    python tests/golden/make_dct_fixed_golden.py

Writes tests/golden/g11_dct_fixed.json with
  matrix_bits   the 64 bit patterns of Floating_point.Eight_point.static_forward_transform_matrix
                (jpeg/model/src/dct.ml:255-337), row-major, as unsigned 64-bit integers;
  scaling       the 32 rows of test_dct_fixed.ml "test scaling" (jpeg/model/test/test_dct_fixed.ml:56-102):
                [i, round i at fixed_prec 3 then clipped to [-128, 127]] for i = -16 .. 15;
  coef_range    the largest and smallest coefficient of either matrix (test_dct_fixed.ml:4-29).
Only data is copied; nothing of the reference's code.
"""
import json
import os
import re

REF = os.environ.get("HVC_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def read(rel):
    with open(os.path.join(REF, rel)) as f:
        return f.read()


def matrix_bits():
    s = read("jpeg/model/src/dct.ml")
    s = s[s.index("static_forward_transform_matrix ="):]
    s = s[:s.index("Int64.float_of_bits")]
    bits = [(-int(h, 16) if neg else int(h, 16)) & (2 ** 64 - 1) for neg, h in re.findall(r"(-?)0x([0-9a-fA-F]+)L", s)]
    assert len(bits) == 64
    return bits


def scaling():
    s = read("jpeg/model/test/test_dct_fixed.ml")
    s = s[s.index('let%expect_test "test scaling"'):]
    s = s[s.index("[%expect"):s.index("|}]")]
    rows = [(int(a), int(b)) for a, b in re.findall(r"^\s*(-?\d+)\s+(-?\d+)\s+[+-]\d", s, re.M)]
    assert [r[0] for r in rows] == list(range(-16, 16))
    return [list(r) for r in rows]


def coef_range():
    s = read("jpeg/model/test/test_dct_fixed.ml")
    m = re.search(r'\("fdct coefficient range" \(max ([\d.]+)\)\s*\(min (-[\d.]+)\)\)', s)
    return [float(m.group(1)), float(m.group(2))]


def main():
    out = {"matrix_bits": matrix_bits(), "scaling": scaling(), "coef_range": coef_range()}
    with open(os.path.join(OUT, "g11_dct_fixed.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
