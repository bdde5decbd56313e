#!/usr/bin/env python3
"""The libjpeg-exact decoder (hvc_set_arithmetic HVC_ARITH_LIBJPEG; csrc/hvc_libjpeg.hip) beside the model's kernels on
BASELINE's configuration-2 workload: a batch of 1080p 4:2:0 coefficient records resident in HBM (1024 frames by default,
`distinct` seeded frames repeated).  One process, the compared calls ALTERNATING step by step, device events on the
context's stream.  Prints one JSON line:

  block_stage   k_islow against k_decode_packed (+ its fix-up kernel): hvc_decode_frames on device memory, the kernel's own
                time from the profiling ring; median and minimum ms, the ratio of the medians, algorithmic bytes (128 B of
                record in + 64 B of pixels out per block) and their share of the 8 TB/s peak
  colour_pass   k_ycc_to_rgb_fancy against k_ycc_to_rgb: hvc_yuv_to_rgb on the decoded planes (interleaved RGB), whole calls
                between device events; algorithmic bytes w * h * 4.5 per frame
  wide_blocks   hvc_last_wide_blocks after the libjpeg block stage (photograph-like content: 0)
  verified      the first `distinct` frames' planes and frame 0's RGB image equal tools/libjpeg_reference.py byte for byte

    python tools/bench_libjpeg.py [--frames 1024] [--steps 20] [--warmup 3] [--distinct 4]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import libjpeg_reference as lj  # noqa: E402

PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=4)
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    from video_coding_amd.synth import synth_frame_pixels
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
    d_rgb = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    blocks = sum(bw * bh for bw, bh, _ in planes)
    order = ("model", "libjpeg")

    # ---- the block stage: the kernel's own time (profiling ring), alternating
    block_ms = {a: [] for a in order}
    ctx.set_profiling(True)
    for step in range(args.warmup + args.steps):
        for a in order:
            ctx.set_arithmetic(a)
            ctx.decode_frames(d_coefs, cfs, qtabs, comps, n, d_pix, pfs)
            ctx.synchronize()
            if step >= args.warmup:
                block_ms[a].append(ctx.last_kernel_ms())
    ctx.set_profiling(False)
    wide = int(ctx.last_wide_blocks())   # (the last call was libjpeg's, and d_pix holds its planes)

    # ---- the colour pass on those planes, whole calls between device events, alternating
    colour_ms = {a: [] for a in order}
    for step in range(args.warmup + args.steps):
        for a in order:
            ctx.set_arithmetic(a)
            ctx.timer_begin()
            ctx.yuv_to_rgb(d_pix, comps, 420, W, H, d_rgb, n_frames=n, yuv_frame_stride=pfs)
            t = ctx.timer_end()
            if step >= args.warmup:
                colour_ms[a].append(t)

    # ---- sampled outputs against the numpy definition
    host = d_distinct.cpu().numpy()
    got_pix = d_pix[:args.distinct].cpu().numpy()
    verified = True
    for f in range(args.distinct):
        ref_planes = lj.record_planes(host[f], qtabs, planes)
        for s, p in zip(specs, ref_planes):
            got = got_pix[f, s["plane_offset"]:s["plane_offset"] + p.size].reshape(p.shape)
            verified &= bool(np.array_equal(got, p))
        if f == 0:
            verified &= bool(np.array_equal(d_rgb[0].cpu().numpy(), lj.planes_to_rgb(ref_planes[0], ref_planes[1], ref_planes[2], 420, W, H)))
    ctx.close()

    def figures(ms, algo):
        out = {}
        for a in order:
            med, low = float(np.median(ms[a])), float(np.min(ms[a]))
            out[a] = {"median_ms": round(med, 4), "min_ms": round(low, 4), "algorithmic_GBps": round(algo / (med * 1e-3) / 1e9, 1),
                      "frac_of_8TBps": round(algo / (med * 1e-3) / PEAK, 4)}
        out["libjpeg_over_model"] = round(float(np.median(ms["libjpeg"]) / np.median(ms["model"])), 4)
        out["libjpeg_over_model_min"] = round(float(np.min(ms["libjpeg"]) / np.min(ms["model"])), 4)
        out["algorithmic_bytes"] = algo
        return out

    print(json.dumps({
        "config": "libjpeg-2", "metric": "k_islow / k_decode_packed and k_ycc_to_rgb_fancy / k_ycc_to_rgb (1080p 4:2:0 batch, HBM-resident)",
        "frames": n, "steps": args.steps, "warmup": args.warmup,
        "block_stage": figures(block_ms, n * blocks * 192), "colour_pass": figures(colour_ms, int(n * W * H * 4.5)),
        "wide_blocks": wide, "verified": verified,
        "how": "planes of the distinct frames and frame 0's RGB image vs tools/libjpeg_reference.py, byte for byte"}))


if __name__ == "__main__":
    main()
