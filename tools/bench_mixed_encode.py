#!/usr/bin/env python3
"""The mixed ENCODE batch (csrc/hvc_mixed_encode.hip, hvc_capi_mixed_encode.hip) measured against the single-geometry entry
points, everything in one process, the compared calls alternating, every output verified first.  Sections (--sections):

  uniform  (a) hvc_encode_frames_mixed on config 5's uniform batch (`--frames` 4K 4:2:0 frames, HBM-resident) against
           hvc_encode_frames on the same frames: device events around k_encode_mixed / k_encode (the profiling ring).  Same
           bytes moved plus 4 bytes of work map per 64 blocks: the ratio is the cost of the table lookups.
  files    (b) a seeded set of `--files` raw frames -- tools/bench_mixed.py's geometry mix: even sides 64 .. 1024, 4:2:0 /
           4:2:2 / 4:4:4, qualities 20 / 50 / 75 / 95, `--distinct` different frames repeated -- through
           hvc_jpeg_encode_batch_mixed against a loop of hvc_jpeg_encode over the same frames, and against the same frames
           sorted by geometry and quality and fed group by group to hvc_jpeg_encode_batch: wall time.
           (c) from the mixed call's stats: the host coder threads' time (entropy_ms_sum / threads) as a share of its wall time.

Prints one JSON line.
    python tools/bench_mixed_encode.py [--sections uniform,files] [--frames 256] [--files 4096] [--distinct 256] [--steps 10] [--threads 16]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

PLANES = [(480, 270, 0), (240, 135, 1), (240, 135, 1)]   # 3840 x 2160 4:2:0
BLOCKS = sum(bw * bh for bw, bh, _ in PLANES)


def section_uniform(args, hvc, torch, ctx):
    from video_coding_amd.synth import synth_frame_pixels
    n, D = args.frames, 4
    qtabs = np.stack([hvc.hvc.quant_table(0, 75), hvc.hvc.quant_table(1, 75)])
    specs, cfs, pfs = hvc.hvc.frame_layout(PLANES)
    comps = hvc.hvc.components(specs)
    src = torch.from_numpy(np.stack([synth_frame_pixels(40 + 8 * f, PLANES) for f in range(D)])).cuda()
    d_pix = src.repeat((n + D - 1) // D, 1)[:n].contiguous()
    d_one = torch.zeros((n, cfs), dtype=torch.int16, device="cuda")
    d_mix = torch.zeros((n, cfs), dtype=torch.int16, device="cuda")
    info = hvc.hvc.JpegInfo()
    info.n_comp, info.n_qtabs, info.coef_count, info.pixel_bytes = len(specs), 2, cfs, pfs
    for t in range(2):
        for k in range(64):
            info.qtabs[t][k] = int(qtabs[t][k])
    for i, s in enumerate(specs):
        L = info.layout[i]
        L.blocks_w, L.blocks_h, L.qtab, L.coef_offset, L.plane_offset, L.stride = (s["blocks_w"], s["blocks_h"], s["qtab"], s["coef_offset"],
                                                                                   s["plane_offset"], s["stride"])
    infos = (hvc.hvc.JpegInfo * n)(*([info] * n))
    co = (C.c_size_t * n)(*[f * cfs for f in range(n)])
    po = (C.c_size_t * n)(*[f * pfs for f in range(n)])
    calls = {"encode_frames": lambda: ctx.encode_frames(d_pix, pfs, qtabs, comps, n, d_one, cfs),
             "encode_frames_mixed": lambda: ctx.encode_frames_mixed(d_pix, po, infos, d_mix, co)}
    for fn in calls.values():
        fn()
    ctx.synchronize()
    ok = bool(torch.equal(d_one, d_mix)) and bool(d_mix.any())
    ctx.set_profiling(True)
    ms = {k: [] for k in calls}
    for step in range(2 + args.steps):
        for k, fn in calls.items():
            fn()
            t = ctx.last_kernel_ms()
            if step >= 2:
                ms[k].append(t)
    ctx.set_profiling(False)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    units = sum(-(-bw * bh // 64) for bw, bh, _ in PLANES) * n
    return {"frames": n, "blocks_per_frame": BLOCKS, "work_units": units, "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
            "TBps": {k: round(n * BLOCKS * 192 / (v * 1e-3) / 1e12, 3) for k, v in med.items()},
            "mixed_over_encode_frames": round(med["encode_frames_mixed"] / med["encode_frames"], 4), "verified": ok}


def mixed_frame_set(distinct, seed=20261018):
    """`distinct` raw frames with tools/bench_mixed.py's draws: even sides 64 .. 1024, three samplings, four qualities; smooth
    content with noise -> (tight Y, U, V as one array each, (width, height, chroma, quality) each)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    frames, keys = [], []
    for _ in range(distinct):
        w, h = (int(rng.integers(32, 513)) * 2 for _ in range(2))
        chroma, quality = (420, 422, 444)[int(rng.integers(0, 3))], (20, 50, 75, 95)[int(rng.integers(0, 4))]
        cw, ch = (w if chroma == 444 else w // 2), (h // 2 if chroma == 420 else h)
        planes = []
        for pw, ph in ((w, h), (cw, ch), (cw, ch)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            p = 128 + 90 * np.sin(xx / float(rng.integers(5, 60)) + yy / float(rng.integers(5, 60))) + rng.integers(-12, 13, size=(ph, pw))
            planes.append(np.clip(p, 0, 255).astype(np.uint8).reshape(-1))
        frames.append(np.concatenate(planes))
        keys.append((w, h, chroma, quality))
    return frames, keys


def section_files(args, hvc, torch, ctx):
    n = args.files
    distinct, dkeys = mixed_frame_set(min(args.distinct, n))
    D = len(distinct)
    frames = [distinct[i % D] for i in range(n)]
    keys = [dkeys[i % D] for i in range(n)]
    lay = hvc.hvc.jpeg_encoder_mixed_layout(keys)
    outs = [np.empty(4 * w * h + 65536, dtype=np.uint8) for w, h, _, _ in keys]
    groups = {}
    for i in range(n):
        groups.setdefault(keys[i], []).append(i)

    def split(i):
        w, h, chroma, _ = keys[i]
        cw, ch = (w if chroma == 444 else w // 2), (h // 2 if chroma == 420 else h)
        f = frames[i]
        return f[:w * h], f[w * h:w * h + cw * ch], f[w * h + cw * ch:]

    def run_mixed():
        return ctx.jpeg_encode_batch_mixed(frames, threads=args.threads, layout=lay, outs=outs)

    def run_loop():
        return [ctx.jpeg_encode(*split(i), *keys[i]) for i in range(n)]

    def run_sorted():
        out = {}
        for (w, h, chroma, quality), idx in groups.items():
            per = max(1, min(len(idx), (64 << 20) // max(1, lay.infos[idx[0]].pixel_bytes)))
            jpgs, _ = ctx.jpeg_encode_batch([frames[i] for i in idx], w, h, chroma, quality, threads=args.threads, frames_per_chunk=per)
            for i, j in zip(idx, jpgs):
                out[i] = j
        return out

    # verification first: every file of the mixed call == hvc_jpeg_encode == its file of the sorted batches
    res = run_mixed()
    st = ctx.last_batch_stats
    stats = {"wall_ms": st.wall_ms, "entropy_ms_sum": st.entropy_ms_sum, "host_prep_ms_sum": st.host_prep_ms_sum,
             "h2d_ms_sum": st.h2d_ms_sum, "kernel_ms_sum": st.kernel_ms_sum, "d2h_ms_sum": st.d2h_ms_sum, "chunks": st.chunks}
    single = [ctx.jpeg_encode(*split(i), *keys[i]) for i in range(D)]
    srt = run_sorted()
    ok = all(r[0] == 0 for r in res)
    for i in range(n):
        ok &= res[i][1] == single[i % D] and srt[i] == single[i % D]
    calls = {"batch_mixed": run_mixed, "loop_of_jpeg_encode": run_loop, "sorted_groups_jpeg_encode_batch": run_sorted}
    wall = {k: [] for k in calls}
    coder_share = []
    for _ in range(max(2, args.steps // 3)):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            if k == "batch_mixed":
                s = ctx.last_batch_stats
                coder_share.append(s.entropy_ms_sum / args.threads / s.wall_ms)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    return {"files": n, "distinct": D, "groups": len(groups), "threads": args.threads,
            "pixel_MB": round(lay.pixel_total / 1e6, 1), "coef_MB": round(2 * lay.coef_total / 1e6, 1),
            "jpeg_MB": round(sum(len(s) for s in single) * (n / D) / 1e6, 1),
            "mixed_chunks": stats["chunks"], "first_call_stats_ms": {k: round(v, 2) for k, v in stats.items() if k != "chunks"},
            "wall_ms": {k: round(v, 2) for k, v in med.items()},
            "wall_ms_min": {k: round(float(np.min(v)), 2) for k, v in wall.items()},
            "files_per_s": {k: round(n / (v * 1e-3)) for k, v in med.items()},
            "loop_over_mixed": round(med["loop_of_jpeg_encode"] / med["batch_mixed"], 3),
            "sorted_over_mixed": round(med["sorted_groups_jpeg_encode_batch"] / med["batch_mixed"], 3),
            "host_coder_share_of_wall": round(float(np.median(coder_share)), 3), "verified": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="uniform,files")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    sections = {"uniform": section_uniform, "files": section_files}
    res = {"kernel_id": hvc.hvc.kernel_build_id()}
    ok = True
    for name in [s for s in args.sections.split(",") if s]:
        ctx = hvc.Context(0)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            res[name] = sections[name](args, hvc, torch, ctx)
        finally:
            ctx.close()
        torch.cuda.empty_cache()
        ok &= res[name]["verified"]
    res["verified"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
