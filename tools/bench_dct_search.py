#!/usr/bin/env python3
"""The precision search of jpeg/bin/dct.ml (`dct search`, hvc_dct_error_search, k_dct_search) on the GPU: the reference's
2 916 round-trip tuples over the default 10^4 generated blocks and over 10^6.  Prints one JSON line per size:

  ms                   one search call (device events around it, after warm-up; mean and min of the timed calls)
  round_trips_per_s    tuples x blocks / ms
  valu_issue_bound     the least time the VALU could issue k_dct_search's instructions in, and its share of ms: per wave
                       and tuple, the ISA's VALU instructions of the inverse pass (every tuple) and of the forward pass
                       (once per change of forward parameters inside a 64-tuple workgroup chunk), each at one wave64
                       instruction per 2 cycles per SIMD, 1 024 SIMDs at 2.4 GHz (MI355X_MICROARCH.md constants)
  checked              tuples whose (max_error, worst_block) equal the numpy restatement of tests/test_dct_fixed_point.py
                       on a sample of tuples (every timed result is the same call's result)

    python tools/bench_dct_search.py [--sizes 10000,1000000] [--steps 5] [--warmup 1] [--check 8]
"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIMDS, CLOCK, CYCLES_PER_VALU = 1024, 2.4e9, 2
KERNEL = "_ZN3hvc12_GLOBAL__N_112k_dct_searchILi2EEE"


def isa_counts():
    """VALU instructions of k_dct_search<round trip>'s forward and inverse basic blocks (the two largest: 1 024 64-bit MADs each)
    and of the per-tuple reduction, from the ISA hipcc makes of hvc_dct_fixed.hip"""
    src = os.path.join(ROOT, "video-coding_amd", "csrc", "hvc_dct_fixed.hip")
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-c", src,
                               "-save-temps=obj", "-o", os.path.join(d, "k.o")], cwd=d, stderr=subprocess.DEVNULL)
        s = open(glob.glob(os.path.join(d, "*gfx950*.s"))[0]).read()
    body = s[re.search(r"^%s\S*:" % KERNEL, s, re.M).end():]
    body = body[:body.index(".Lfunc_end")]
    blocks = []
    for part in re.split(r"\n\.LBB\S+:[^\n]*", body):
        v = [ln.split()[0] for ln in part.split("\n") if ln.strip().startswith("v_")]
        blocks.append((sum(x.startswith("v_mad_") and "64" in x for x in v), sum(x.startswith("v_max") for x in v), len(v)))
    passes = sorted(sorted(blocks, key=lambda b: b[2])[-2:], key=lambda b: b[1])
    assert all(b[0] >= 1024 for b in passes), passes
    return passes[0][2], passes[1][2]   # the inverse pass is the one that takes max |x - y| of its outputs


def forward_runs(tuples, chunk=64):
    """forward passes k_dct_search makes per block: one per change of (fwd_rom, fwd_tp) inside each chunk"""
    n = 0
    for c0 in range(0, len(tuples), chunk):
        prev = None
        for t in tuples[c0:c0 + chunk]:
            n += t[:2] != prev
            prev = t[:2]
    return n


def blocks_np(seed, rng, first, n):
    """hvc_dct_blocks vectorised (uint64 arithmetic wraps mod 2^64)"""
    with np.errstate(over="ignore"):
        i = np.arange(first, first + n, dtype=np.uint64)[:, None] * np.uint64(32) + np.arange(1, 33, dtype=np.uint64)
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * i
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    lo, hi = z & np.uint64(0xFFFFFFFF), z >> np.uint64(32)
    w = np.stack([lo, hi], axis=-1).reshape(n, 64)
    return ((w * np.uint64(2 * rng)) >> np.uint64(32)).astype(np.int64).reshape(n, 8, 8) - rng


def restated(tuples, n, seed=0, chunk=100000):
    from test_dct_fixed_point import round_trip_errors
    best = [(-1, 0)] * len(tuples)
    for b0 in range(0, n, chunk):
        x = blocks_np(seed, 128, b0, min(chunk, n - b0))
        for k, t in enumerate(tuples):
            e = round_trip_errors(x, *t)
            m = int(e.max())
            if m > best[k][0]:
                best[k] = (m, b0 + int(np.argmax(e == m)))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,1000000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", type=int, default=8, help="tuples restated on the CPU per size")
    args = ap.parse_args()
    import video_coding_amd as hvc
    from video_coding_amd.__main__ import dct_search_configs
    from test_dct_fixed_point import blocks
    tuples = dct_search_configs()
    cfgs = hvc.hvc.dct_configs([("round_trip",) + t for t in tuples])
    assert np.array_equal(blocks_np(3, 128, 5, 7), blocks(3, 128, 5, 7))
    fwd, inv = isa_counts()
    per_wave_tuple = inv + fwd * forward_runs(tuples) / len(tuples)
    ctx = hvc.Context(0)
    rng = np.random.default_rng(1)
    try:
        for n in [int(v) for v in args.sizes.split(",")]:
            for _ in range(args.warmup):
                ctx.dct_error_search(cfgs, 0, 128, 0, n)
            ms = []
            for _ in range(args.steps):
                ctx.timer_begin()
                e, w = ctx.dct_error_search(cfgs, 0, 128, 0, n)
                ms.append(ctx.timer_end())
            pick = sorted(rng.choice(len(tuples), size=args.check, replace=False).tolist())
            want = restated([tuples[k] for k in pick], n)
            ok = sum((int(e[k]), int(w[k])) == want[j] for j, k in enumerate(pick))
            bound_s = (n / 64) * len(tuples) * per_wave_tuple * CYCLES_PER_VALU / (SIMDS * CLOCK)
            mean = float(np.mean(ms))
            print(json.dumps({
                "metric": "dct_search", "tuples": len(tuples), "blocks": n, "ms": round(mean, 3),
                "ms_min": round(float(np.min(ms)), 3), "steps": args.steps,
                "round_trips_per_s": len(tuples) * n / (mean / 1e3),
                "valu_issue_bound": {"valu_per_wave_tuple": round(per_wave_tuple, 1), "fwd_pass_valu": fwd,
                                     "inv_pass_valu": inv, "ms": round(bound_s * 1e3, 3),
                                     "share": round(bound_s * 1e3 / mean, 3)},
                "checked": "%d/%d" % (ok, len(pick)), "max_error_range": [int(e.min()), int(e.max())]}), flush=True)
            if ok != len(pick):
                sys.exit(1)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
