#!/usr/bin/env python3
"""Default against per-file optimised Huffman tables on configuration 5's workload (4K 4:2:0 frames at q75, the frame
generator of config 5 end to end, `distinct` seeded frames repeated), both in one process, runs alternating:

  coder       the GPU Huffman coder alone on HBM-resident coefficient records, frames_per_chunk frames per call
              (hvc_huffman_encode_frames / _optimised), timed by device events on the context's stream
  e2e_gpu     raw frames in, files out through hvc_jpeg_encode_batch_gpu, in Gpixel/s (hvc_batch_stats.wall_ms)
  e2e_host    the same through hvc_jpeg_encode_batch (host coder threads)
  bytes       total bytes of the files written, and the share the optimised tables save

Every file is verified: each distinct frame's optimised file equals the host composition of its coefficient record
(hvc_huffman_optimal_tables + hvc_jpeg_entropy_encode_tables), the record being the one the default-table file carries;
every repeat equals its distinct frame's file; the GPU coder's segments equal the host's.  Prints one JSON line.

    python tools/bench_huffman_optimise.py [--frames 256] [--distinct 8] [--steps 3] [--chunk 16] [--threads 16]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    from video_coding_amd.synth import synth_pixels
    H_ = hvc.hvc
    W, H = 3840, 2160
    ctx = hvc.Context(0)
    distinct = []
    for f in range(args.distinct):
        y, u, v = synth_pixels(110 + f, H, W), synth_pixels(120 + f, H // 2, W // 2), synth_pixels(130 + f, H // 2, W // 2)
        distinct.append(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]))
    frames = [distinct[i % args.distinct] for i in range(args.frames)]
    info = H_.jpeg_encoder_layout(W, H, 420, 75)
    px = W * H * args.frames

    def e2e(mode, gpu):
        ctx.set_huffman_tables(mode)
        jpegs, st = ctx.jpeg_encode_batch(frames, W, H, 420, 75, threads=args.threads, frames_per_chunk=args.chunk,
                                          gpu_entropy=gpu)
        ctx.set_huffman_tables("default")
        return jpegs, st.wall_ms

    # warm-up: rings and scratch of both modes
    for mode in ("default", "optimised"):
        for gpu in (True, False):
            ctx.set_huffman_tables(mode)
            ctx.jpeg_encode_batch(frames[:2 * args.chunk], W, H, 420, 75, threads=args.threads, frames_per_chunk=args.chunk,
                                  gpu_entropy=gpu)
    ctx.set_huffman_tables("default")

    # -- end to end, alternating ---------------------------------------------------------------------------------------
    ms = {(m, g): [] for m in ("default", "optimised") for g in (True, False)}
    files = {}
    for _ in range(args.steps):
        for gpu in (True, False):
            for mode in ("default", "optimised"):
                jpegs, wall = e2e(mode, gpu)
                ms[(mode, gpu)].append(wall)
                files[(mode, gpu)] = jpegs
    # -- verification ---------------------------------------------------------------------------------------------------
    ok = True
    for key, jpegs in files.items():
        ok &= all(jpegs[f] == jpegs[f % args.distinct] for f in range(args.frames))
    ok &= files[("default", True)][:args.distinct] == files[("default", False)][:args.distinct]
    ok &= files[("optimised", True)][:args.distinct] == files[("optimised", False)][:args.distinct]
    recs = []
    for f in range(args.distinct):
        _, rec = H_.jpeg_entropy_decode(files[("default", True)][f])
        rec = np.ascontiguousarray(rec.reshape(-1)[:info.coef_count])
        recs.append(rec)
        ok &= files[("optimised", True)][f] == H_.jpeg_entropy_encode(info, rec, "optimised")
    # -- the GPU coder alone on HBM-resident records -----------------------------------------------------------------
    n = args.chunk
    d_coefs = torch.from_numpy(np.stack([recs[f % args.distinct] for f in range(n)]).reshape(-1)).cuda()
    cap = n * info.coef_count * 2
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    specs = (H_.HuffSpec * (4 * n))()
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    L = hvc.lib()

    def coder(mode):
        if mode == "default":
            return L.hvc_huffman_encode_frames(ctx._h, C.byref(info), d_coefs.data_ptr(), info.coef_count, n,
                                               d_out.data_ptr(), cap, d_off.data_ptr(), 1)
        return L.hvc_huffman_encode_frames_optimised(ctx._h, C.byref(info), d_coefs.data_ptr(), info.coef_count, n,
                                                     d_out.data_ptr(), cap, d_off.data_ptr(), specs, 1)

    coder_ms = {"default": [], "optimised": []}
    seg_ok = True
    for step in range(args.steps * 4 + 2):
        for mode in ("default", "optimised"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = coder(mode)
            e1.record()
            torch.cuda.synchronize()
            assert r == 0, r
            if step >= 2:
                coder_ms[mode].append(e0.elapsed_time(e1))
            if step == 0:
                o = d_off.cpu().numpy()
                data = d_out[:int(o[-1])].cpu().numpy().tobytes()
                for f in range(args.distinct if args.distinct < n else n):
                    fs = [specs[4 * f + t].to_pair() for t in range(4)] if mode == "optimised" else None
                    jpg = H_.jpeg_entropy_encode(info, recs[f % args.distinct], fs)
                    head = H_.jpeg_header(info, fs)
                    seg_ok &= data[int(o[f]):int(o[f + 1])] == jpg[len(head):-2]
    ctx.reset_stream()
    ok &= seg_ok
    med = lambda v: float(np.median(v))
    bytes_d = sum(map(len, files[("default", True)]))
    bytes_o = sum(map(len, files[("optimised", True)]))
    res = {
        "workload": "config 5: %d x %dx%d 4:2:0 q75, %d distinct frames" % (args.frames, W, H, args.distinct),
        "coder_frames_per_call": n,
        "coder_ms": {m: round(med(v), 3) for m, v in coder_ms.items()},
        "coder_Gpixel_s": {m: round(n * W * H / (med(v) * 1e-3) / 1e9, 1) for m, v in coder_ms.items()},
        "coder_ratio_optimised_over_default": round(med(coder_ms["default"]) / med(coder_ms["optimised"]), 3),
        "e2e_gpu_Gpixel_s": {m: round(px / (med(ms[(m, True)]) * 1e-3) / 1e9, 2) for m in ("default", "optimised")},
        "e2e_host_Gpixel_s": {m: round(px / (med(ms[(m, False)]) * 1e-3) / 1e9, 2) for m in ("default", "optimised")},
        "e2e_gpu_ratio": round(med(ms[("default", True)]) / med(ms[("optimised", True)]), 3),
        "e2e_host_ratio": round(med(ms[("default", False)]) / med(ms[("optimised", False)]), 3),
        "wall_ms_runs": {"%s_%s" % (m, "gpu" if g else "host"): [round(x, 1) for x in v] for (m, g), v in ms.items()},
        "bytes": {"default": bytes_d, "optimised": bytes_o},
        "saved_percent": round(100.0 * (bytes_d - bytes_o) / bytes_d, 2),
        "verified": bool(ok),
    }
    ctx.close()
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
