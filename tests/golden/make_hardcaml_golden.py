#!/usr/bin/env python3
"""Extract the data the Hardcaml RTL twin is checked against (G9) from the
reference's tests and model data.  CPU only; run once where the reference
exists:

    python tests/golden/make_hardcaml_golden.py

Writes tests/golden/g9_hardcaml.json with
  rom           the 64 ROM integers of Dct.Make(Idct_config): round_nearest(4096 * M),
                M = the transpose of the x86 static forward matrix (jpeg/model/src/dct.ml:255-346,
                hardcaml/src/dct.ml:75-83), row-major;
  idct          the Idct module's RTL simulation vector (jpeg/hardcaml/test/test_dct.ml:251-300):
                dct_inputs, transpose (4 fractional bits) and pixels (before the level shift,
                saturated to [-128, 127]), each 8 x 8 row-major;
  mouse_blocks  block_number, max_reconstructed_diff and the RTL pixels of Mouse480 blocks 0-5
                (jpeg/hardcaml/test/test_decoder_accelerator.ml:209-376).
Only data is copied; nothing of the reference's code.
"""
import json
import math
import os
import re
import struct

REF = os.environ.get("HVC_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))


def read(rel):
    with open(os.path.join(REF, rel)) as f:
        return f.read()


def ints(s):
    return [int(x) for x in re.findall(r"-?\d+", s)]


def rom():
    s = read("jpeg/model/src/dct.ml")
    s = s[s.index("static_forward_transform_matrix ="):]
    s = s[:s.index("|> Array.map")]
    bits = [int(v, 16) * (-1 if neg else 1) for neg, v in
            ((m.group(1) == "-", m.group(2)) for m in re.finditer(r"(-?)0x([0-9a-f]+)L", s))]
    assert len(bits) == 64
    fwd = [struct.unpack("<d", struct.pack("<q", b))[0] for b in bits]   # Int64.float_of_bits
    # inverse = transpose forward; OCaml's Float.round_nearest rounds half away from zero
    rnd = lambda f: int(math.floor(abs(f) * 4096.0 + 0.5)) * (1 if f >= 0 else -1)
    return [rnd(fwd[c * 8 + r]) for r in range(8) for c in range(8)]


def idct_vector():
    s = read("jpeg/hardcaml/test/test_dct.ml")
    s = s[s.index("module Idct = struct"):]
    s = s[s.index("((dct_inputs"):]
    m = re.search(r"\(\(dct_inputs(.*?)\(transpose(.*?)\(pixels(.*?)\)\)\)\)", s, re.S)
    d, t, p = (ints(m.group(i)) for i in (1, 2, 3))
    assert len(d) == len(t) == len(p) == 64
    return {"source": "jpeg/hardcaml/test/test_dct.ml:251-300", "dct_inputs": d, "transpose": t, "pixels": p}


def mouse_blocks():
    s = read("jpeg/hardcaml/test/test_decoder_accelerator.ml")
    s = s[s.index("((width 480) (height 320))"):]
    out = []
    for m in re.finditer(r"\(\(block_number (\d+)\) \(max_reconstructed_diff (\d+)\)\s*\(pixels\s*(\(.*?\)\))\)", s, re.S):
        px = [int(v, 16) for v in re.findall(r"\b[0-9a-f]{2}\b", m.group(3))]
        assert len(px) == 64
        out.append({"block_number": int(m.group(1)), "max_reconstructed_diff": int(m.group(2)), "pixels": px})
    assert [b["block_number"] for b in out] == list(range(6)), [b["block_number"] for b in out]
    return out


def main():
    g = {"source": "jpeg/model/src/dct.ml:255-346; jpeg/hardcaml/test/test_dct.ml; "
                   "jpeg/hardcaml/test/test_decoder_accelerator.ml:209-376",
         "rom": rom(), "idct": idct_vector(), "mouse_blocks": mouse_blocks()}
    with open(os.path.join(OUT, "g9_hardcaml.json"), "w") as f:
        json.dump(g, f, indent=1)
        f.write("\n")
    print("rom row 0..1:", g["rom"][:16])


if __name__ == "__main__":
    main()
