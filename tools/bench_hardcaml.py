#!/usr/bin/env python3
"""The Hardcaml RTL twin (hvc_set_arithmetic HVC_ARITH_HARDCAML, k_hardcaml) on BASELINE's configuration-2 workload: a batch
of 1080p 4:2:0 coefficient records resident in HBM (1024 frames by default, `distinct` seeded frames repeated), decoded to
pixel records in HBM.  Prints one JSON line:

  kernel_ms            k_hardcaml per launch (device events around the kernel, mean of the timed steps)
  value                Mpixel/s of that
  algorithmic_bytes    128 B of record in + 64 B of pixels out per block, and their rate's fraction of the 8 TB/s peak
  model                the model path (k_decode_packed + its fix-up kernel) on the same batch in the same process
  divergence           hvc_decode_frames_divergence over the batch (model into scratch + the twin's compare form), whole
                       calls timed with device events
  checksum             K5 (hvc_checksum_records) of every output record against the checksums of the numpy restatement
                       (tests/test_hardcaml_twin.py) of the distinct frames: `verified`

    python tools/bench_hardcaml.py [--frames 1024] [--steps 20] [--warmup 3] [--distinct 8]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=8)
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    from video_coding_amd.synth import synth_frame_pixels
    from test_hardcaml_twin import hardcaml_blocks
    W, H = 1920, 1080
    planes = [(240, 136, 0), (120, 68, 1), (120, 68, 1)]
    qtabs = np.stack([hvc.hvc.quant_table(0, 75), hvc.hvc.quant_table(1, 75)])
    specs, cfs, pfs = hvc.hvc.frame_layout(planes)
    comps = hvc.hvc.components(specs)
    ctx = hvc.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    src = torch.from_numpy(np.stack([synth_frame_pixels(40 + 8 * f, planes) for f in range(args.distinct)])).cuda()
    d_distinct = torch.zeros((args.distinct, cfs), dtype=torch.int16, device="cuda")
    ctx.encode_frames(src, pfs, qtabs, comps, args.distinct, d_distinct, cfs)
    n = args.frames
    d_coefs = d_distinct.repeat((n + args.distinct - 1) // args.distinct, 1)[:n].contiguous()
    d_pix = torch.zeros((n, pfs), dtype=torch.uint8, device="cuda")
    blocks = sum(bw * bh for bw, bh, _ in planes)
    algo = n * blocks * 192

    def timed(arith):
        ctx.set_arithmetic(arith)
        ctx.set_profiling(True)
        for _ in range(args.warmup):
            ctx.decode_frames(d_coefs, cfs, qtabs, comps, n, d_pix, pfs)
        torch.cuda.synchronize()
        for _ in range(args.steps):
            ctx.decode_frames(d_coefs, cfs, qtabs, comps, n, d_pix, pfs)
        torch.cuda.synchronize()
        ms = float(np.mean(ctx.kernel_ms_history(min(args.steps, 64))))
        ctx.set_profiling(False)
        return ms

    model_ms = timed("model")
    k_ms = timed("hardcaml")   # (last: d_pix holds the twin's output for the check below)

    # K5 over every output record against the restatement of the distinct frames
    host = d_distinct.cpu().numpy()
    want = []
    for f in range(args.distinct):
        rec = np.zeros(pfs, dtype=np.uint8)
        for s in specs:
            bw, bh = s["blocks_w"], s["blocks_h"]
            blk = host[f, s["coef_offset"]:s["coef_offset"] + bw * bh * 64].reshape(bh, bw, 64)
            px = hardcaml_blocks(blk, qtabs[s["qtab"]]).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
            rec[s["plane_offset"]:s["plane_offset"] + bw * bh * 64] = px.reshape(-1)
        want.append("%016x" % int(ctx.checksum_records(rec, pfs, 1)[0]))
    got = ["%016x" % int(x) for x in ctx.checksum_records(d_pix, pfs, n)]
    verified = all(got[r] == want[r % args.distinct] for r in range(n))

    # the divergence call, whole calls (model into scratch + the twin's compare form)
    d_diff = torch.zeros((n, blocks), dtype=torch.uint8, device="cuda")
    for _ in range(max(1, args.warmup)):
        ctx.decode_divergence(d_coefs, cfs, qtabs, comps, n, d_diff, blocks)
    steps_div = max(1, args.steps // 4)
    ctx.synchronize()
    ctx.timer_begin()
    for _ in range(steps_div):
        ctx.decode_divergence(d_coefs, cfs, qtabs, comps, n, d_diff, blocks)
    div_ms = ctx.timer_end() / steps_div
    hist = np.bincount(d_diff.view(-1).cpu().numpy(), minlength=256)
    ctx.close()

    rate = lambda ms: algo / (ms * 1e-3)
    print(json.dumps({
        "config": "hardcaml-2", "metric": "Mpixel/s decoded by the RTL twin (1080p 4:2:0 batch, HBM-resident)", "frames": n,
        "value": round(n * W * H / (k_ms * 1e-3) / 1e6, 1), "unit": "Mpixel/s", "kernel_ms": round(k_ms, 4),
        "algorithmic_bytes": algo, "algorithmic_GBps": round(rate(k_ms) / 1e9, 1), "frac_of_8TBps": round(rate(k_ms) / PEAK, 4),
        "model": {"kernel_ms": round(model_ms, 4), "value": round(n * W * H / (model_ms * 1e-3) / 1e6, 1),
                  "frac_of_8TBps": round(rate(model_ms) / PEAK, 4)},
        "divergence": {"call_ms": round(div_ms, 4), "Mpixel_per_s": round(n * W * H / (div_ms * 1e-3) / 1e6, 1),
                       "max_diff_histogram": {str(i): int(c) for i, c in enumerate(hist) if c}},
        "checksum": {"records": n, "distinct": want, "how": "K5 of every record vs the numpy restatement of the distinct frames",
                     "verified": verified}}))


if __name__ == "__main__":
    main()
