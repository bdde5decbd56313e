#!/usr/bin/env python3
"""Restart intervals written by the encoder, on configuration 5's workload (4K 4:2:0 frames at q75, the frame generator
of config 5 end to end, `distinct` seeded frames repeated), everything in one process, runs alternating:

  coder       the GPU Huffman coder alone on HBM-resident coefficient records, frames_per_chunk frames per call
              (hvc_huffman_encode_frames_restart), default and optimised tables, no interval against Ri in --intervals,
              timed by device events on the context's stream
  e2e_gpu     raw frames in, files out through hvc_jpeg_encode_batch_gpu, in Gpixel/s (hvc_batch_stats.wall_ms)
  e2e_host    the same through hvc_jpeg_encode_batch (host coder threads)
  bytes       total bytes of the files written and what the intervals add in per cent
  reader      hvc_jpeg_entropy_decode_gpu with hvc_set_restart_markers on over --reader-files restart files against the
              same call over the plain files of the same frames (wall time per call; Ri in --reader-intervals only: the
              GPU reader takes at most 65535 intervals per call); used_gpu says whether the GPU reader kept them

Every file is verified: each distinct frame's file equals the host composition of its coefficient record
(hvc_jpeg_entropy_encode_restart), the record being the one the plain file carries; every repeat equals its distinct
frame's file; the GPU coder's segments equal the host's; the reader returns the records.  Prints one JSON line.

    python tools/bench_restart_encode.py [--frames 256] [--distinct 8] [--steps 3] [--chunk 16] [--threads 16]
                                         [--intervals 240,16,1] [--reader-intervals 240,16] [--reader-files 32]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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
    ap.add_argument("--intervals", default="240,16,1")
    ap.add_argument("--reader-intervals", dest="reader_intervals", default="240,16")
    ap.add_argument("--reader-files", dest="reader_files", type=int, default=32)
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    from video_coding_amd.synth import synth_pixels
    H_ = hvc.hvc
    W, H = 3840, 2160
    ris = [0] + [int(x) for x in args.intervals.split(",") if x]
    reader_ris = [int(x) for x in args.reader_intervals.split(",") if x]
    modes = [(t, ri) for t in ("default", "optimised") for ri in ris]
    ctx = hvc.Context(0)
    distinct = []
    for f in range(args.distinct):
        y, u, v = synth_pixels(110 + f, H, W), synth_pixels(120 + f, H // 2, W // 2), synth_pixels(130 + f, H // 2, W // 2)
        distinct.append(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]))
    frames = [distinct[i % args.distinct] for i in range(args.frames)]
    info = H_.jpeg_encoder_layout(W, H, 420, 75)
    px = W * H * args.frames
    name = lambda t, ri: "%s_ri%d" % (t, ri) if ri else t

    def e2e(tables, ri, gpu, fr=frames):
        ctx.set_huffman_tables(tables)
        ctx.set_restart_interval(ri)
        try:
            jpegs, st = ctx.jpeg_encode_batch(fr, W, H, 420, 75, threads=args.threads, frames_per_chunk=args.chunk, gpu_entropy=gpu)
        finally:
            ctx.set_huffman_tables("default")
            ctx.set_restart_interval(0)
        return jpegs, st.wall_ms

    for t, ri in modes:  # warm-up: rings and scratch of every mode
        for gpu in (True, False):
            e2e(t, ri, gpu, frames[:2 * args.chunk])

    # -- end to end, alternating ---------------------------------------------------------------------------------------
    ms = {(t, ri, g): [] for t, ri in modes for g in (True, False)}
    files = {}
    for _ in range(args.steps):
        for gpu in (True, False):
            for t, ri in modes:
                jpegs, wall = e2e(t, ri, gpu)
                ms[(t, ri, gpu)].append(wall)
                files[(t, ri, gpu)] = jpegs
    # -- verification ---------------------------------------------------------------------------------------------------
    ok = True
    for jpegs in files.values():
        ok &= all(jpegs[f] == jpegs[f % args.distinct] for f in range(args.frames))
    recs = []
    for f in range(args.distinct):
        _, rec = H_.jpeg_entropy_decode(files[("default", 0, True)][f])
        recs.append(np.ascontiguousarray(rec.reshape(-1)[:info.coef_count]))
    for t, ri in modes:
        ok &= files[(t, ri, True)][:args.distinct] == files[(t, ri, False)][:args.distinct]
        for f in range(args.distinct):
            ok &= files[(t, ri, True)][f] == H_.jpeg_entropy_encode(info, recs[f], None if t == "default" else "optimised",
                                                                   restart_interval=ri)
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

    def coder(t, ri):
        return L.hvc_huffman_encode_frames_restart(ctx._h, C.byref(info), d_coefs.data_ptr(), info.coef_count, n, ri,
                                                   H_.HVC_HUFF[t], d_out.data_ptr(), cap, d_off.data_ptr(), specs, 1)

    coder_ms = {m: [] for m in modes}
    seg_ok = True
    for step in range(args.steps * 4 + 2):
        for t, ri in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = coder(t, ri)
            e1.record()
            torch.cuda.synchronize()
            assert r == 0, r
            if step >= 2:
                coder_ms[(t, ri)].append(e0.elapsed_time(e1))
            if step == 0:
                o = d_off.cpu().numpy()
                data = d_out[:int(o[-1])].cpu().numpy().tobytes()
                for f in range(min(args.distinct, n)):
                    fs = [specs[4 * f + k].to_pair() for k in range(4)] if t == "optimised" else None
                    jpg = H_.jpeg_entropy_encode(info, recs[f % args.distinct], fs, restart_interval=ri)
                    head = H_.jpeg_header(info, fs, restart_interval=ri)
                    seg_ok &= data[int(o[f]):int(o[f + 1])] == jpg[len(head):-2]
    ctx.reset_stream()
    ok &= seg_ok
    # -- the reader's side: the GPU reader over restart files against the plain files of the same frames -----------------------------
    ctx.set_restart_markers(True)
    nr = min(args.reader_files, args.frames)
    reader_ms, reader_used = {}, {}
    sets = {"plain": files[("default", 0, True)][:nr]}
    for ri in reader_ris:
        if ("default", ri, True) in files:
            sets["ri%d" % ri] = files[("default", ri, True)][:nr]
    for k in sets:
        reader_ms[k] = []
    for step in range(args.steps + 1):
        for k, fs in sets.items():
            t0 = time.perf_counter()
            _, got, used = ctx.jpeg_entropy_decode_gpu(fs, device=True)
            dt = (time.perf_counter() - t0) * 1e3
            if step:
                reader_ms[k].append(dt)
            else:
                reader_used[k] = used
                ok &= all(np.array_equal(got[f][:info.coef_count], recs[f % args.distinct]) for f in range(min(nr, args.distinct)))
    ctx.set_restart_markers(False)
    med = lambda v: float(np.median(v))
    nbytes = {name(t, ri): sum(map(len, files[(t, ri, True)])) for t, ri in modes}
    res = {
        "workload": "config 5: %d x %dx%d 4:2:0 q75, %d distinct frames" % (args.frames, W, H, args.distinct),
        "coder_frames_per_call": n,
        "coder_ms": {name(*m): round(med(v), 3) for m, v in coder_ms.items()},
        "coder_ratio_over_no_interval": {name(t, ri): round(med(coder_ms[(t, 0)]) / med(coder_ms[(t, ri)]), 3) for t, ri in modes if ri},
        "e2e_gpu_Gpixel_s": {name(t, ri): round(px / (med(ms[(t, ri, True)]) * 1e-3) / 1e9, 2) for t, ri in modes},
        "e2e_host_Gpixel_s": {name(t, ri): round(px / (med(ms[(t, ri, False)]) * 1e-3) / 1e9, 2) for t, ri in modes},
        "bytes": nbytes,
        "added_percent": {name(t, ri): round(100.0 * (nbytes[name(t, ri)] - nbytes[name(t, 0)]) / nbytes[name(t, 0)], 3)
                          for t, ri in modes if ri},
        "reader_files_per_call": nr,
        "reader_wall_ms": {k: round(med(v), 2) for k, v in reader_ms.items()},
        "reader_used_gpu": reader_used,
        "verified": bool(ok),
    }
    ctx.close()
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
