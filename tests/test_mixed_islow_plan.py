"""The table records of the libjpeg-exact mixed block stage (hvc::mixed_islow_pairs_build, csrc/hvc_mixed_plan.cpp; read by
k_islow_mixed, csrc/hvc_mixed_libjpeg.hip), without a GPU: through the stand-alone program
tests/host_harness/mixed_islow_plan_harness.cpp, which runs the builder behind hvc::mixed_plan_build under AddressSanitizer and
UndefinedBehaviorSanitizer (a CPU-only g++ build: tests/host_harness/Makefile.mixed_islow).  Nothing loaded into Python runs
under a sanitizer.  A record is IslowParams::qq's form: 32 words q[2i] | q[2i+1] << 16 in zig-zag order, all 16 bits of every
entry; one per distinct table of the plan, in plan.tables order."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mixed_islow") / "mixed_islow_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.mixed_islow", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


def run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.split()


@pytest.mark.parametrize("seed", [20261020, 7])
def test_seeded_sets_with_16_bit_entries_and_shared_tables(harness, seed):
    """entries from 1 to 65535, duplicates within and across frames: every pair word, one record per distinct table, in
    plan.tables order (the harness checks each set; here: that sets had tables to share and shared them)"""
    out = run(harness, "random", seed, 300)
    assert out[:2] == ["ok", "300"] and out[2] == "tables" and out[4] == "shared"
    assert int(out[3]) >= 300 and int(out[5]) > 0


@pytest.mark.parametrize("n_tables", [1, 5, 513, 2049])
def test_more_distinct_tables_than_any_fixed_array(harness, n_tables):
    assert run(harness, "distinct", 99, n_tables) == ["ok", "tables", str(n_tables)]


def test_an_empty_plan_gives_no_record(harness):
    assert run(harness, "empty") == ["ok", "empty"]


@pytest.mark.parametrize("table", ["ramp", "ends", "all_65535", "random"])
def test_the_words_of_one_table(harness, table):
    """the words themselves, against numpy: word i = q[2i] | q[2i+1] << 16"""
    q = {"ramp": np.arange(1, 65), "ends": np.where(np.arange(64) % 2, 65535, 1), "all_65535": np.full(64, 65535),
         "random": np.random.default_rng(5).integers(1, 65536, 64)}[table].astype(np.uint32)
    out = run(harness, "dump", *q.tolist())
    assert out[0] == "pairs" and len(out) == 33
    assert [int(v) for v in out[1:]] == (q[0::2] | (q[1::2] << 16)).tolist()
