"""The hand-off between a batch pipeline's host workers and its orchestrating thread (csrc/hvc_feed.h), without a GPU: the
stand-alone program tests/host_harness/feed_harness.cpp drives a real worker pool and the feed with a fake orchestrator, in
two CPU-only g++ builds (tests/host_harness/Makefile.feed) -- one that reports data races, one that reports memory and
undefined-behaviour errors.  Nothing loaded into Python runs under a sanitizer.  Every scenario runs 200 times in one process,
each time followed by a plain batch on the same pool; a deadlock is the subprocess timeout, a broken invariant an abort."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "TSAN_OPTIONS": "halt_on_error=1", "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1",
       "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
ENV.pop("HVC_POOL_FAIL_AFTER", None)
REPS = 200
TIMEOUT = 60    # seconds per scenario

SCENARIOS = [
    "plain",               # 10 items in chunks of 3 (the last one ragged, more chunks than slots); 1, 2, 8, 16 workers
    "pairs",               # items claimed two at a time across chunk boundaries
    "unequal",             # chunks of 1, 4, 1, 2, 5 items
    "slow_fast",           # the orchestrator slow to release, then fast
    "worker_error",        # an item of chunk 0, of chunk RING, of the last chunk fails; the first error stays
    "orchestrator_fails",  # finish(rc != 0) while workers wait for a slot; rc wins
    "throws",              # a worker body throws std::bad_alloc: HVC_E_OUT_OF_MEMORY, no termination
    "leaves_early",        # the feed goes out of scope without finish(): HVC_E_INTERNAL, the workers end
    "refused",             # HVC_POOL_FAIL_AFTER: the pool refuses a thread, HVC_E_SYSTEM, the threads that exist go on
]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("feed") / "feed_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.feed", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("build", ["tsan", "asan"])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_feed_scenario(harness, scenario, build):
    env = dict(ENV, HVC_POOL_FAIL_AFTER="2") if scenario == "refused" else ENV
    r = subprocess.run([harness + "." + build, scenario, str(REPS)], capture_output=True, text=True, env=env, timeout=TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    words = r.stdout.split()
    assert words[:3] == ["ok", scenario, str(REPS)], r.stdout[-2000:]
    print(scenario, build, words[3], "ms")
