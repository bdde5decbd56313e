#!/usr/bin/env python3
"""Extract the data the Hardcaml RTL encoder twin is checked against (G10) from the
reference's tests and model data.  CPU only; run once where the reference exists:

    python tests/golden/make_hardcaml_encoder_golden.py REFERENCE_DIR      (or HVC_REFERENCE=REFERENCE_DIR)

Writes tests/golden/g10_hardcaml_encoder.json with
  rom_forward   the 64 ROM integers of Dct.Make(Dct_config): round_nearest(4096 * F),
                F = the x86 static forward matrix (jpeg/model/src/dct.ml:255-346), row-major;
  dct           the forward Dct module's RTL simulation vector (jpeg/hardcaml/test/test_dct.ml:131-250):
                dct_inputs (level-shifted pixels), transpose (4 fractional bits) and pixels (the
                12-bit coefficients), each 8 x 8 row-major;
  quant_cases   the quantiser's hand-checked cases (jpeg/hardcaml/test/test_quant.ml:175-201);
  quant_table   the random table test_quant.ml:118-121 prints;
  luma95        Quant_tables.(scale luma 95) as test_encoder_accelerator.ml:11-17 prints it.
Only data is copied; nothing of the reference's code.
"""
import json
import math
import os
import re
import struct
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HVC_REFERENCE", "")
OUT = os.path.dirname(os.path.abspath(__file__))


def read(rel):
    with open(os.path.join(REF, rel)) as f:
        return f.read()


def ints(s):
    return [int(x) for x in re.findall(r"-?\d+", s)]


def rom_forward():
    s = read("jpeg/model/src/dct.ml")
    s = s[s.index("static_forward_transform_matrix ="):]
    s = s[:s.index("|> Array.map")]
    bits = [int(v, 16) * (-1 if neg else 1) for neg, v in
            ((m.group(1) == "-", m.group(2)) for m in re.finditer(r"(-?)0x([0-9a-f]+)L", s))]
    assert len(bits) == 64
    fwd = [struct.unpack("<d", struct.pack("<q", b))[0] for b in bits]   # Int64.float_of_bits
    rnd = lambda f: int(math.floor(abs(f) * 4096.0 + 0.5)) * (1 if f >= 0 else -1)   # Float.round_nearest
    return [rnd(f) for f in fwd]


def dct_vector():
    s = read("jpeg/hardcaml/test/test_dct.ml")
    s = s[s.index("module Dct = struct"):s.index("module Idct = struct")]
    s = s[s.index("((dct_inputs"):]
    m = re.search(r"\(\(dct_inputs(.*?)\(transpose(.*?)\(pixels(.*?)\)\)\)\)", s, re.S)
    d, t, p = (ints(m.group(i)) for i in (1, 2, 3))
    assert len(d) == len(t) == len(p) == 64
    return {"source": "jpeg/hardcaml/test/test_dct.ml:131-250", "dct_inputs": d, "transpose": t, "pixels": p}


def quant_data():
    s = read("jpeg/hardcaml/test/test_quant.ml")
    t = s[s.index("(qtab\n"):]
    table = ints(t[:t.index("|}")])
    assert len(table) == 64
    cases = []
    for m in re.finditer(r"test \((-?\d+)\) (\d+);|test (\d+) (\d+);", s):
        d, q = (m.group(1), m.group(2)) if m.group(1) else (m.group(3), m.group(4))
        rest = s[m.end():]
        e = re.search(r"\(expected (-?\d+)\)", rest)
        cases.append({"d": int(d), "t": int(q), "expected": int(e.group(1))})
    assert [(c["d"], c["t"], c["expected"]) for c in cases] == [(-188, 2, -94), (709, 1, 709)], cases
    return table, cases


def luma95():
    s = read("jpeg/hardcaml/test/test_encoder_accelerator.ml")
    s = s[s.index("(qtable\n"):]
    t = ints(s[:s.index("|}")])
    assert len(t) == 64
    return t


def main():
    if not REF or not os.path.isdir(os.path.join(REF, "jpeg", "hardcaml")):
        sys.exit("usage: make_hardcaml_encoder_golden.py REFERENCE_DIR (the hardcaml video-coding checkout)")
    table, cases = quant_data()
    g = {"source": "jpeg/model/src/dct.ml:255-346; jpeg/hardcaml/test/test_dct.ml:131-250; "
                   "jpeg/hardcaml/test/test_quant.ml:118-121, 175-201; jpeg/hardcaml/test/test_encoder_accelerator.ml:11-17",
         "rom_forward": rom_forward(), "dct": dct_vector(), "quant_cases": cases, "quant_table": table,
         "luma95": luma95()}
    with open(os.path.join(OUT, "g10_hardcaml_encoder.json"), "w") as f:
        json.dump(g, f, indent=1)
        f.write("\n")
    print("rom_forward rows 0..1:", g["rom_forward"][:16])


if __name__ == "__main__":
    main()
