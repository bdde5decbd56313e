#!/usr/bin/env python3
"""The mixed batch at 1/2, 1/4 and 1/8 size (csrc/hvc_mixed_scaled.hip, hvc_capi_mixed.hip) measured against the
single-geometry scaled entry points, everything in one process, the compared calls alternating, every output verified first.
Sections (--sections, default all), each at scale_denom 2, 4 and 8:

  uniform  (a) hvc_decode_frames_mixed_scaled on the headline's uniform batch (`--frames` 1080p 4:2:0 records, HBM-resident)
           against hvc_decode_frames_scaled on the same records: device events around k_decode_mixed_scaled / k_decode_scaled
           (the profiling ring).  The ratio is the cost of taking the decomposition from device memory.
  files    (b) the seeded set of tools/bench_mixed.py (`--files` files, `--distinct` different ones) through
           hvc_jpeg_decode_batch_mixed_scaled (host output) against the full-size hvc_jpeg_decode_batch_mixed and against a
           loop of hvc_jpeg_decode_scaled over the same files: wall time, and the bytes of output.
  rgb      (c) the same set through hvc_jpeg_decode_batch_mixed_scaled_rgb against a loop of hvc_jpeg_decode_scaled_rgb.

The host Huffman reader bounds the file pipelines at every scale: (b) and (c) show what the scaled form saves in output
memory and download, not a faster block stage.  Prints one JSON line.
    python tools/bench_mixed_scaled.py [--sections uniform,files,rgb] [--frames 1024] [--files 4096] [--distinct 256] [--steps 10]
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
from bench_mixed import BLOCKS, PLANES, mixed_file_set  # noqa: E402

SCALES = (2, 4, 8)


def section_uniform(args, hvc, torch, ctx):
    from video_coding_amd.synth import synth_frame_pixels
    n, D = args.frames, 4
    qtabs = np.stack([hvc.hvc.quant_table(0, 75), hvc.hvc.quant_table(1, 75)])
    specs, cfs, pfs = hvc.hvc.frame_layout(PLANES)
    comps = hvc.hvc.components(specs)
    src = torch.from_numpy(np.stack([synth_frame_pixels(40 + 8 * f, PLANES) for f in range(D)])).cuda()   # config 2's frames
    d_distinct = torch.zeros((D, cfs), dtype=torch.int16, device="cuda")
    ctx.encode_frames(src, pfs, qtabs, comps, D, d_distinct, cfs)
    d_coefs = d_distinct.repeat((n + D - 1) // D, 1)[:n].contiguous()
    del src
    full = hvc.hvc.JpegInfo()
    full.n_comp, full.n_qtabs, full.coef_count, full.pixel_bytes = len(specs), 2, cfs, pfs
    for t in range(2):
        for k in range(64):
            full.qtabs[t][k] = int(qtabs[t][k])
    for i, s in enumerate(specs):
        L = full.layout[i]
        L.blocks_w, L.blocks_h, L.qtab, L.coef_offset, L.plane_offset, L.stride = (s["blocks_w"], s["blocks_h"], s["qtab"], s["coef_offset"],
                                                                                   s["plane_offset"], s["stride"])
    co = (C.c_size_t * n)(*[f * cfs for f in range(n)])
    out = {"frames": n, "blocks_per_frame": BLOCKS, "scales": {}}
    ok = True
    for scale in SCALES:
        N = 8 // scale
        info = hvc.hvc.jpeg_scaled_info(full, scale)   # tight scaled planes
        sfs = info.pixel_bytes
        sspecs = [dict(s, plane_offset=info.layout[i].plane_offset, stride=info.layout[i].stride) for i, s in enumerate(specs)]
        scomps = hvc.hvc.components(sspecs)
        infos = (hvc.hvc.JpegInfo * n)(*([info] * n))
        po = (C.c_size_t * n)(*[f * sfs for f in range(n)])
        d_pix = torch.zeros((n, sfs), dtype=torch.uint8, device="cuda")
        d_mix = torch.zeros((n, sfs), dtype=torch.uint8, device="cuda")
        calls = {"decode_frames_scaled": lambda: ctx.decode_frames_scaled(d_coefs, cfs, qtabs, scomps, n, scale, d_pix, sfs),
                 "decode_frames_mixed_scaled": lambda: ctx.decode_frames_mixed_scaled(d_coefs, co, infos, scale, d_mix, po)}
        wide = []
        for fn in calls.values():
            fn()
            wide.append(ctx.last_wide_blocks())
        ctx.synchronize()
        ok &= bool(torch.equal(d_pix, d_mix)) and wide[0] == wide[1]
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
        moved = n * BLOCKS * ((128 if N > 1 else 32) + N * N)   # bytes read (N = 1: the sector that holds the DC) + written
        out["scales"][str(scale)] = {"ms": {k: round(v, 4) for k, v in med.items()},
                                     "ms_min": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
                                     "TBps": {k: round(moved / (v * 1e-3) / 1e12, 3) for k, v in med.items()},
                                     "wide_blocks": int(wide[0]),
                                     "mixed_over_decode_frames_scaled": round(med["decode_frames_mixed_scaled"] / med["decode_frames_scaled"], 4)}
        del d_pix, d_mix
    out["verified"] = bool(ok)
    return out


def timed(calls, reps, ctx):
    wall = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return {k: float(np.median(v)) for k, v in wall.items()}


def section_files(args, hvc, torch, ctx, rgb=False):
    n = args.files
    distinct, _ = mixed_file_set(ctx, min(args.distinct, n))
    files = [distinct[i % len(distinct)] for i in range(n)]
    reps = max(2, args.steps // 5)
    out = {"files": n, "distinct": len(distinct), "threads": args.threads, "scales": {}}
    ok = True
    if rgb:
        flay = hvc.hvc.jpeg_mixed_rgb_layout(files)
        fbuf = np.zeros(flay.total_bytes, dtype=np.uint8)
        full = lambda: ctx.jpeg_decode_batch_mixed_rgb(files, threads=args.threads, rgb_layout=flay, rgb=fbuf)   # noqa: E731
    else:
        flay = hvc.hvc.jpeg_mixed_layout(files)
        fbuf = np.zeros(flay.total_bytes, dtype=np.uint8)
        full = lambda: ctx.jpeg_decode_batch_mixed(files, threads=args.threads, layout=flay, pixels=fbuf)   # noqa: E731
    out["full_size_MB"] = round(flay.total_bytes / 1e6, 1)
    for scale in SCALES:
        if rgb:
            lay = hvc.hvc.jpeg_mixed_scaled_rgb_layout(files, scale)
            buf = np.zeros(lay.total_bytes, dtype=np.uint8)
            mixed = lambda: ctx.jpeg_decode_batch_mixed_scaled_rgb(files, scale, threads=args.threads, rgb_layout=lay, rgb=buf)   # noqa: E731
            loop = lambda: [ctx.jpeg_decode_scaled_rgb(f, scale)[1] for f in files]   # noqa: E731
            single = [ctx.jpeg_decode_scaled_rgb(f, scale)[1] for f in distinct]
            res = mixed()
            ok &= all(r[0] == 0 and np.array_equal(r[2], single[i % len(distinct)]) for i, r in enumerate(res))
        else:
            lay = hvc.hvc.jpeg_mixed_scaled_layout(files, scale)
            buf = np.zeros(lay.total_bytes, dtype=np.uint8)
            mixed = lambda: ctx.jpeg_decode_batch_mixed_scaled(files, scale, threads=args.threads, layout=lay, pixels=buf)   # noqa: E731
            loop = lambda: [ctx.jpeg_decode_scaled(f, scale)[1] for f in files]   # noqa: E731
            single = [ctx.jpeg_decode_scaled(f, scale)[1] for f in distinct]
            res = mixed()
            ok &= all(r[0] == 0 for r in res)
            for i in range(n):
                off = lay.pixel_offsets[i]
                ok &= bool(np.array_equal(buf[off:off + lay.scaled[i].pixel_bytes], single[i % len(distinct)]))
        st = ctx.last_batch_stats
        names = ("batch_mixed_scaled", "batch_mixed_full_size", "loop_of_jpeg_decode_scaled")
        med = timed(dict(zip(names, (mixed, full, loop))), reps, ctx)
        out["scales"][str(scale)] = {"output_MB": round(lay.total_bytes / 1e6, 1), "chunks": st.chunks,
                                     "entropy_ms_sum": round(st.entropy_ms_sum, 1), "wall_ms": {k: round(v, 2) for k, v in med.items()},
                                     "files_per_s": {k: round(n / (v * 1e-3)) for k, v in med.items()},
                                     "loop_over_mixed_scaled": round(med[names[2]] / med[names[0]], 3),
                                     "full_size_over_mixed_scaled": round(med[names[1]] / med[names[0]], 3)}
    out["verified"] = bool(ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="uniform,files,rgb")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    sections = {"uniform": section_uniform, "files": section_files,
                "rgb": lambda a, h, t, c: section_files(a, h, t, c, rgb=True)}
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
