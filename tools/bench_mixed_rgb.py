#!/usr/bin/env python3
"""The mixed batch to RGB (csrc/hvc_mixed_rgb.hip, hvc_mixed_rgb_plan.cpp, hvc_capi_mixed.hip) measured against the
single-geometry entry points, everything in one process, the compared calls alternating, every output verified first.
Sections (--sections, default all):

  uniform  (a) k_ycc_to_rgb_mixed (hvc_yuv_to_rgb_mixed) against k_ycc_to_rgb (hvc_yuv_to_rgb) on the headline's uniform batch:
           the planes of `--frames` 1080p 4:2:0 frames, HBM-resident, interleaved output; device events around each call.
           Same bytes moved plus 4 bytes of work map per 64 lanes: the ratio is the cost of the table lookups.  Verified by K5
           checksums of the two outputs, frame by frame.
  files    (b) the seeded file set of tools/bench_mixed.py through hvc_jpeg_decode_batch_mixed_rgb (device output) against a
           loop of hvc_jpeg_decode_rgb, and against hvc_jpeg_decode_batch_mixed to device memory followed by one
           hvc_yuv_to_rgb per file: wall time.  Verified against hvc_jpeg_decode_rgb file by file.
           (c) the same call with row_align 1 (tight rows: 8-byte stores only where width % 8 == 0) against row_align 8.

Prints one JSON line.
    python tools/bench_mixed_rgb.py [--sections uniform,files] [--frames 1024] [--files 4096] [--distinct 256] [--steps 10] [--threads 16]
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

from bench_mixed import PLANES, mixed_file_set  # noqa: E402

W, H = 1920, 1080


def section_uniform(args, hvc, torch, ctx):
    n, D = args.frames, 4
    specs, _, pfs = hvc.hvc.frame_layout(PLANES)
    comps = hvc.hvc.components(specs)
    rng = np.random.Generator(np.random.PCG64(7))
    src = torch.from_numpy(rng.integers(0, 256, size=(D, pfs), dtype=np.uint8)).cuda()
    d_yuv = src.repeat((n + D - 1) // D, 1)[:n].contiguous()
    fb = 3 * W * H
    d_one = torch.zeros((n, fb), dtype=torch.uint8, device="cuda")
    d_mix = torch.zeros((n, fb), dtype=torch.uint8, device="cuda")
    info = hvc.hvc.JpegInfo()
    info.width, info.height, info.n_comp, info.n_qtabs, info.pixel_bytes = W, H, 3, 1, pfs
    for i, s in enumerate(specs):
        info.comp[i].hscale = info.comp[i].vscale = 2 if i == 0 else 1
        L = info.layout[i]
        L.blocks_w, L.blocks_h, L.plane_offset, L.stride = s["blocks_w"], s["blocks_h"], s["plane_offset"], s["stride"]
    infos = (hvc.hvc.JpegInfo * n)(*([info] * n))
    yo = (C.c_size_t * n)(*[f * pfs for f in range(n)])
    ro = (C.c_size_t * n)(*[f * fb for f in range(n)])
    calls = {"yuv_to_rgb": lambda: ctx.yuv_to_rgb(d_yuv, comps, 420, W, H, d_one, n_frames=n, yuv_frame_stride=pfs),
             "yuv_to_rgb_mixed": lambda: ctx.yuv_to_rgb_mixed(d_yuv, yo, infos, d_mix, ro)}
    for fn in calls.values():
        fn()
    ctx.synchronize()
    ok = bool(np.array_equal(ctx.checksum_records(d_one, fb, n), ctx.checksum_records(d_mix, fb, n)))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {k: [] for k in calls}
    for step in range(2 + args.steps):
        for k, fn in calls.items():
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            if step >= 2:
                ms[k].append(ev[0].elapsed_time(ev[1]))
    ctx.set_profiling(True)   # the mixed kernel alone, through the profiling ring
    own = []
    for _ in range(args.steps):
        calls["yuv_to_rgb_mixed"]()
        own.append(ctx.last_kernel_ms())
    ctx.set_profiling(False)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    moved = n * (W * H * 3 // 2 + fb)
    return {"frames": n, "work_units": n * (-(-(W // 8) * (H // 2) // 64)), "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min": {k: round(float(np.min(v)), 4) for k, v in ms.items()}, "mixed_kernel_ms": round(float(np.median(own)), 4),
            "TBps": {k: round(moved / (v * 1e-3) / 1e12, 3) for k, v in med.items()},
            "mixed_over_yuv_to_rgb": round(med["yuv_to_rgb_mixed"] / med["yuv_to_rgb"], 4), "verified": ok}


def section_files(args, hvc, torch, ctx):
    n = args.files
    distinct, keys = mixed_file_set(ctx, min(args.distinct, n))
    files = [distinct[i % len(distinct)] for i in range(n)]
    single = [ctx.jpeg_decode_rgb(f)[1] for f in distinct]
    lays = {ra: hvc.hvc.jpeg_mixed_rgb_layout(files, "interleaved", 0, ra) for ra in (1, 8)}
    bufs = {ra: torch.zeros(max(lays[ra].total_bytes, 8), dtype=torch.uint8, device="cuda") for ra in (1, 8)}
    ylay = hvc.hvc.jpeg_mixed_layout(files)
    d_planes = torch.zeros(max(ylay.total_bytes, 8), dtype=torch.uint8, device="cuda")
    d_rgb2 = torch.zeros(max(lays[1].total_bytes, 8), dtype=torch.uint8, device="cuda")
    comps = [hvc.hvc.components([dict(blocks_w=ylay.infos[i].layout[k].blocks_w, blocks_h=ylay.infos[i].layout[k].blocks_h,
                                      plane_offset=ylay.infos[i].layout[k].plane_offset, stride=ylay.infos[i].layout[k].stride)
                                 for k in range(3)]) for i in range(len(distinct))]

    def run_mixed(ra):
        return ctx.jpeg_decode_batch_mixed_rgb(files, threads=args.threads, device=True, rgb_layout=lays[ra], rgb=bufs[ra])

    def run_loop():
        return [ctx.jpeg_decode_rgb(f)[1] for f in files]

    def run_yuv_then_each():
        ctx.jpeg_decode_batch_mixed(files, threads=args.threads, device=True, layout=ylay, pixels=d_planes)
        for i in range(n):
            w, h, chroma, _ = keys[i % len(distinct)]
            off, roff = ylay.pixel_offsets[i], lays[1].rgb_offsets[i]
            ctx.yuv_to_rgb(d_planes[off:off + ylay.infos[i].pixel_bytes], comps[i % len(distinct)], chroma, w, h,
                           d_rgb2[roff:roff + 3 * w * h])

    ok = True
    for ra in (1, 8):
        res = run_mixed(ra)
        ctx.synchronize()
        host = bufs[ra].cpu().numpy()
        ok &= all(r[0] == 0 for r in res)
        for i in range(n):
            info = lays[ra].infos[i]
            got = hvc.hvc.rgb_view(host, lays[ra].rgb_offsets[i], lays[ra].rgb_row_strides[i], info.width, info.height, 0)
            ok &= bool(np.array_equal(got, single[i % len(distinct)]))
    st = ctx.last_batch_stats
    run_yuv_then_each()
    ctx.synchronize()
    host = d_rgb2.cpu().numpy()
    for i in range(n):
        info = lays[1].infos[i]
        ok &= bool(np.array_equal(hvc.hvc.rgb_view(host, lays[1].rgb_offsets[i], 0, info.width, info.height, 0), single[i % len(distinct)]))
    calls = {"batch_mixed_rgb": lambda: run_mixed(1), "batch_mixed_rgb_row_align_8": lambda: run_mixed(8),
             "batch_mixed_then_yuv_to_rgb_per_file": run_yuv_then_each, "loop_of_jpeg_decode_rgb": run_loop}
    wall = {k: [] for k in calls}
    kms = {1: [], 8: []}
    for _ in range(max(2, args.steps // 3)):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            if k.startswith("batch_mixed_rgb"):
                kms[8 if k.endswith("8") else 1].append(ctx.last_batch_stats.kernel_ms_sum)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    aligned = sum(1 for i in range(n) if keys[i % len(distinct)][0] % 8 == 0)
    return {"files": n, "distinct": len(distinct), "threads": args.threads, "rgb_MB": round(lays[1].total_bytes / 1e6, 1),
            "mixed_chunks": st.chunks, "files_with_width_on_8": aligned, "wall_ms": {k: round(v, 2) for k, v in med.items()},
            "files_per_s": {k: round(n / (v * 1e-3)) for k, v in med.items()},
            "kernel_ms_sum": {"row_align_1": round(float(np.median(kms[1])), 3), "row_align_8": round(float(np.median(kms[8])), 3)},
            "loop_over_mixed_rgb": round(med["loop_of_jpeg_decode_rgb"] / med["batch_mixed_rgb"], 3),
            "yuv_then_each_over_mixed_rgb": round(med["batch_mixed_then_yuv_to_rgb_per_file"] / med["batch_mixed_rgb"], 3),
            "row_align_1_over_8": round(med["batch_mixed_rgb"] / med["batch_mixed_rgb_row_align_8"], 3), "verified": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="uniform,files")
    ap.add_argument("--frames", type=int, default=1024)
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
