"""The host arithmetic of the libjpeg-exact encoder (csrc/hvc_libjpeg_encode_plan.cpp: the quantiser's division magics, the
dummy blocks' source index, the replicating pad), without a GPU: through the stand-alone program
tests/host_harness/libjpeg_encode_plan_harness.cpp under AddressSanitizer and UndefinedBehaviorSanitizer (a CPU-only g++
build: tests/host_harness/Makefile.libjpeg_encode).  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import libjpeg_encode_reference as ler  # noqa: E402

HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("libjpeg_encode") / "libjpeg_encode_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.libjpeg_encode", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


def run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.split()


def test_every_divisor_against_every_numerator(harness):
    """q in 1 .. 255 x |t| in 0 .. the proved bound, both signs, against C's /"""
    k = ler.spec_constants()
    assert run(harness, "magics") == ["ok", "magics", str(2 * k["HVC_FI_Q_MAX"] * (k["HVC_FI_T_MAX"] + 1))]


def test_the_table_words_are_natural_order_words_of_zigzag_entries(harness):
    out = run(harness, "tables")
    assert out[0] == "tables" and len(out) == 1 + 4 * 64
    got = np.array([int(v) for v in out[1:]], dtype=np.int64).reshape(2, 64, 2)
    q = np.stack([np.arange(1, 65), 255 - np.arange(64)])[:, ler.ZF]  # the entry of natural position k
    assert np.array_equal(got[..., 1], 4 * q)
    assert np.array_equal(got[..., 0], -(-(1 << 26) // (8 * q)))


def test_dummy_sources_closed_form_against_the_walk(harness):
    out = run(harness, "dummies", 12, 12)
    assert out[:2] == ["ok", "dummies"] and int(out[2]) > 1000 and int(out[3]) > 100000


def test_the_walk_is_the_numpy_definitions(harness):
    """the harness holds the closed form to the C++ walk; the numpy definition (held to Pillow) walks the same way"""
    for bw, bh, rw, rh, h, v in [(4, 4, 3, 3, 2, 2), (6, 4, 5, 3, 2, 2), (4, 2, 3, 2, 2, 1), (8, 8, 5, 6, 4, 4), (2, 4, 2, 3, 1, 2)]:
        for by in range(bh):
            for bx in range(bw):
                sx, sy = ler.dummy_source(bx, by, rw, rh, h, v)
                last = bx // h * h + h - 1
                want = (min(last, rw - 1), rh - 1) if by >= rh else (min(bx, rw - 1), by)
                assert (sx, sy) == want


def test_the_colour_pass_lane_grid(harness):
    out = run(harness, "rgb")
    assert out[:2] == ["ok", "rgb"] and int(out[2]) > 5000


def test_the_replicating_pad_stays_inside_its_record(harness):
    out = run(harness, "pad")
    assert out[:2] == ["ok", "pad"] and int(out[2]) > 1000
