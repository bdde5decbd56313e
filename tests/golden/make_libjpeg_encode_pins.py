"""Writes tests/golden/libjpeg_encode_pins.json: per case of tests/libjpeg_encode_cases.py the SHA-256 of the coefficient
record (int16, little endian) of the file libjpeg-turbo (through Pillow) writes from the case's samples with our tables.
tests/test_libjpeg_encode_reference.py holds the numpy definition against Pillow itself where Pillow is installed and
against these pins everywhere; tests/test_gpu_libjpeg_encode.py holds the GPU's records against them.

    python tests/golden/make_libjpeg_encode_pins.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import libjpeg_encode_cases as lc  # noqa: E402


def pins():
    out = {}
    for case in lc.plane_cases() + lc.rgb_cases():
        _, coefs = lc.file_record(lc.pillow_file(case), case[5])
        out[case[0]] = lc.sha256(coefs.astype("<i2"))
    return out


if __name__ == "__main__":
    with open(lc.PINS, "w") as f:
        json.dump(pins(), f, indent=1, sort_keys=True)
        f.write("\n")
