#!/usr/bin/env python3
"""The Hardcaml RTL encoder twin (hvc_set_encode_arithmetic HVC_ARITH_HARDCAML, k_hardcaml_encode) on BASELINE's
configuration-5 workload: a batch of 4K 4:2:0 pixel records resident in HBM (256 frames by default, `distinct` seeded
frames repeated), encoded at quality 75 to coefficient records in HBM.  Prints one JSON line:

  kernel_ms            k_hardcaml_encode per launch (device events around the kernel, mean of the timed steps)
  value                Mpixel/s of that
  algorithmic_bytes    64 B of pixels in + 128 B of record out per block, and their rate's fraction of the 8 TB/s peak
  model                k_encode on the same batch in the same process, timed in alternation with the twin
  divergence           hvc_encode_frames_divergence over the batch (k_encode into scratch + the twin's compare form),
                       whole calls timed with device events, and the histogram of its bytes
  checksum             K5 (hvc_checksum_records) of every output record against the checksums of the numpy restatement
                       (tests/test_hardcaml_encoder_twin.py) of the distinct frames: `verified`

    python tools/bench_hardcaml_encoder.py [--frames 256] [--steps 20] [--warmup 3] [--distinct 4]
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
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the twin and k_encode")
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    from video_coding_amd.synth import synth_frame_pixels
    from test_hardcaml_encoder_twin import hardcaml_encode_blocks
    W, H = 3840, 2160
    planes = [(480, 270, 0), (240, 135, 1), (240, 135, 1)]
    qtabs = np.stack([hvc.hvc.quant_table(0, 75), hvc.hvc.quant_table(1, 75)])
    specs, cfs, pfs = hvc.hvc.frame_layout(planes)
    comps = hvc.hvc.components(specs)
    ctx = hvc.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    host = np.stack([synth_frame_pixels(50 + 8 * f, planes) for f in range(args.distinct)])
    n = args.frames
    d_pix = torch.from_numpy(host).cuda().repeat((n + args.distinct - 1) // args.distinct, 1)[:n].contiguous()
    d_coefs = torch.zeros((n, cfs), dtype=torch.int16, device="cuda")
    blocks = sum(bw * bh for bw, bh, _ in planes)
    algo = n * blocks * 192

    def timed(arith):
        ctx.set_encode_arithmetic(arith)
        ctx.set_profiling(True)
        for _ in range(args.warmup):
            ctx.encode_frames(d_pix, pfs, qtabs, comps, n, d_coefs, cfs)
        torch.cuda.synchronize()
        for _ in range(args.steps):
            ctx.encode_frames(d_pix, pfs, qtabs, comps, n, d_coefs, cfs)
        torch.cuda.synchronize()
        ms = float(np.mean(ctx.kernel_ms_history(min(args.steps, 64))))
        ctx.set_profiling(False)
        return ms

    model, twin = [], []
    for _ in range(max(1, args.rounds)):
        model.append(timed("model"))
        twin.append(timed("hardcaml"))   # (last: d_coefs holds the twin's output for the check below)
    k_ms, model_ms = float(np.median(twin)), float(np.median(model))

    # K5 over every output record against the restatement of the distinct frames
    want = []
    for f in range(args.distinct):
        rec = np.zeros(cfs, dtype=np.int16)
        for s in specs:
            bw, bh = s["blocks_w"], s["blocks_h"]
            plane = host[f, s["plane_offset"]:s["plane_offset"] + s["stride"] * bh * 8].reshape(bh * 8, s["stride"])
            blk = plane[:, :bw * 8].reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
            rec[s["coef_offset"]:s["coef_offset"] + bw * bh * 64] = hardcaml_encode_blocks(blk, qtabs[s["qtab"]]).reshape(-1)
        want.append("%016x" % int(ctx.checksum_records(rec, cfs * 2, 1)[0]))
    got = ["%016x" % int(x) for x in ctx.checksum_records(d_coefs, cfs * 2, n)]
    verified = all(got[r] == want[r % args.distinct] for r in range(n))

    # the divergence call, whole calls (k_encode into scratch + the twin's compare form)
    d_diff = torch.zeros((n, blocks), dtype=torch.uint8, device="cuda")
    for _ in range(max(1, args.warmup)):
        ctx.encode_divergence(d_pix, pfs, qtabs, comps, n, d_diff, blocks)
    steps_div = max(1, args.steps // 4)
    ctx.synchronize()
    ctx.timer_begin()
    for _ in range(steps_div):
        ctx.encode_divergence(d_pix, pfs, qtabs, comps, n, d_diff, blocks)
    div_ms = ctx.timer_end() / steps_div
    hist = np.bincount(d_diff.view(-1).cpu().numpy(), minlength=256)
    ctx.close()

    rate = lambda ms: algo / (ms * 1e-3)
    print(json.dumps({
        "config": "hardcaml-encoder-5", "metric": "Mpixel/s encoded by the RTL encoder twin (4K 4:2:0 batch, q75, HBM-resident)",
        "frames": n, "value": round(n * W * H / (k_ms * 1e-3) / 1e6, 1), "unit": "Mpixel/s", "kernel_ms": round(k_ms, 4),
        "kernel_ms_rounds": [round(x, 4) for x in twin],
        "algorithmic_bytes": algo, "algorithmic_GBps": round(rate(k_ms) / 1e9, 1), "frac_of_8TBps": round(rate(k_ms) / PEAK, 4),
        "model": {"kernel_ms": round(model_ms, 4), "kernel_ms_rounds": [round(x, 4) for x in model],
                  "value": round(n * W * H / (model_ms * 1e-3) / 1e6, 1), "frac_of_8TBps": round(rate(model_ms) / PEAK, 4)},
        "divergence": {"call_ms": round(div_ms, 4), "Mpixel_per_s": round(n * W * H / (div_ms * 1e-3) / 1e6, 1),
                       "max_diff_histogram": {str(i): int(c) for i, c in enumerate(hist) if c}},
        "checksum": {"records": n, "distinct": want, "how": "K5 of every record vs the numpy restatement of the distinct frames",
                     "verified": verified}}))


if __name__ == "__main__":
    main()
