"""The host plan of the uniform GPU Huffman reader (csrc/hvc_hdec_plan.h), without a GPU: the restart-interval decision, the
layout of a ring slot of hvc_jpeg_decode_batch_gpu and the index fill of a chunk, through the stand-alone program
tests/host_harness/hdec_plan_harness.cpp under AddressSanitizer and UndefinedBehaviorSanitizer (a CPU-only g++ build:
tests/host_harness/Makefile.hdec_plan).  The harness allocates every array at the size the layout states and writes it the way
the pipeline does, so a wrong offset is a sanitizer report; it also restates the arithmetic the pipeline carried before the plan
existed and compares every value.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hdec_plan") / "hdec_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.hdec_plan", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


def run(harness, what):
    r = subprocess.run([harness, what], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and not any(ln.startswith("FAILED") for ln in lines), r.stdout[-3000:]
    return lines


def test_chunk_layouts_and_index_fills_over_the_sweep(harness):
    """C in {1, 2, 5} x cnt in 1..C x ipf in {1, 2, 7} x max_file in {1, 127, 128, 129, 389} x segment lengths from {0, 1, 127,
    128, 129, all the room} x tables of their own for no / every / every other file: regions in order, disjoint and ending at
    meta_words; the travelling prefix exactly ecs_off | sub_off | tabset_of; every reader frame inside its file's region of the
    segment slot; sub_off strictly increasing up to the returned total, at most C * nsub_max; tabset_of 0 or 1 + f."""
    lines = run(harness, "sweep")
    w = lines[-2].split()
    assert w[0] == "sweep" and int(w[2]) == 3 * 3 * 5
    # per layout and table pattern: every combination of six lengths up to four reader frames, 1296 drawn ones beyond
    per = {n: min(6 ** n, 1296) for n in range(1, 36)}
    want = sum(3 * per[cnt * ipf] for C in (1, 2, 5) for cnt in range(1, C + 1) for ipf in (1, 2, 7)) * 5
    assert int(w[4]) == want


def test_sizes_at_two_to_the_31_are_refused(harness):
    assert run(harness, "limits")[-2] == "limits checked"


def test_the_restart_decision_at_its_edges_and_both_ceilings(harness):
    assert run(harness, "restart")[-2] == "restart checked"
