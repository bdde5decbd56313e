#!/usr/bin/env python3
"""The mixed batch (csrc/hvc_mixed.hip, hvc_capi_mixed.hip) measured against the single-geometry entry points, everything in
one process, the compared calls alternating, every output verified first.  Sections (--sections, default all):

  uniform  (a) hvc_decode_frames_mixed on the headline's uniform batch (`--frames` 1080p 4:2:0 records, HBM-resident) against
           hvc_decode_frames on the same records: device events around k_decode_mixed / k_decode_packed (the profiling
           ring).  Same bytes moved plus 4 bytes of work map per 64 blocks: the ratio is the cost of the table lookups.
  files    (b) a seeded set of `--files` files -- sides between 64 and 1024, 4:2:0 / 4:2:2 / 4:4:4, qualities 20 / 50 / 75 / 95,
           `--distinct` different files repeated -- through hvc_jpeg_decode_batch_mixed (host output) against a loop of
           hvc_jpeg_decode over the same files: wall time.
           (c) the same files sorted by geometry and tables and fed group by group to hvc_jpeg_decode_batch: wall time.

Prints one JSON line.
    python tools/bench_mixed.py [--sections uniform,files] [--frames 1024] [--files 4096] [--distinct 256] [--steps 10] [--threads 16]
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

PLANES = [(240, 136, 0), (120, 68, 1), (120, 68, 1)]   # 1920 x 1080 4:2:0
BLOCKS = sum(bw * bh for bw, bh, _ in PLANES)


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
    d_pix = torch.zeros((n, pfs), dtype=torch.uint8, device="cuda")
    d_mix = torch.zeros((n, pfs), dtype=torch.uint8, device="cuda")
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
    calls = {"decode_frames": lambda: ctx.decode_frames(d_coefs, cfs, qtabs, comps, n, d_pix, pfs),
             "decode_frames_mixed": lambda: ctx.decode_frames_mixed(d_coefs, co, infos, d_mix, po)}
    for fn in calls.values():
        fn()
    ctx.synchronize()
    ok = bool(torch.equal(d_pix, d_mix)) and ctx.last_wide_blocks() == 0
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
            "mixed_over_decode_frames": round(med["decode_frames_mixed"] / med["decode_frames"], 4), "verified": ok}


def mixed_file_set(ctx, distinct, seed=20261018):
    """`distinct` files: even sides 64 .. 1024, three samplings, four qualities; smooth content with noise"""
    rng = np.random.Generator(np.random.PCG64(seed))
    files, keys = [], []
    for _ in range(distinct):
        w, h = (int(rng.integers(32, 513)) * 2 for _ in range(2))
        chroma, quality = (420, 422, 444)[int(rng.integers(0, 3))], (20, 50, 75, 95)[int(rng.integers(0, 4))]
        cw, ch = (w if chroma == 444 else w // 2), (h // 2 if chroma == 420 else h)
        planes = []
        for pw, ph in ((w, h), (cw, ch), (cw, ch)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            p = 128 + 90 * np.sin(xx / float(rng.integers(5, 60)) + yy / float(rng.integers(5, 60))) + rng.integers(-12, 13, size=(ph, pw))
            planes.append(np.clip(p, 0, 255).astype(np.uint8))
        files.append(ctx.jpeg_encode(planes[0], planes[1], planes[2], w, h, chroma, quality))
        keys.append((w, h, chroma, quality))
    return files, keys


def section_files(args, hvc, torch, ctx):
    n = args.files
    distinct, keys = mixed_file_set(ctx, min(args.distinct, n))
    files = [distinct[i % len(distinct)] for i in range(n)]
    lay = hvc.hvc.jpeg_mixed_layout(files)
    pixels = np.zeros(lay.total_bytes, dtype=np.uint8)
    # (c): groups of one geometry and one set of tables, each with a buffer of its own
    groups = {}
    for i in range(n):
        groups.setdefault(keys[i % len(distinct)], []).append(i)
    gbuf = {k: np.zeros((len(v), lay.infos[v[0]].pixel_bytes), dtype=np.uint8) for k, v in groups.items()}

    def run_mixed():
        return ctx.jpeg_decode_batch_mixed(files, threads=args.threads, layout=lay, pixels=pixels)

    def run_loop():
        return [ctx.jpeg_decode(f)[1] for f in files]

    def run_sorted():
        for k, idx in groups.items():
            ctx.jpeg_decode_batch([files[i] for i in idx], gbuf[k], gbuf[k].shape[1], threads=args.threads,
                                  frames_per_chunk=max(1, min(len(idx), (64 << 20) // max(1, 2 * lay.infos[idx[0]].coef_count))))

    # verification first: every file of the mixed call == hvc_jpeg_decode == its frame of the sorted batches
    res = run_mixed()
    single = [ctx.jpeg_decode(f)[1] for f in distinct]
    run_sorted()
    ok = all(r[0] == 0 for r in res)
    for i in range(n):
        off, nb = lay.pixel_offsets[i], lay.infos[i].pixel_bytes
        ok &= bool(np.array_equal(pixels[off:off + nb], single[i % len(distinct)]))
    for k, idx in groups.items():
        for j, i in enumerate(idx):
            ok &= bool(np.array_equal(gbuf[k][j], single[i % len(distinct)]))
    st = ctx.last_batch_stats
    calls = {"batch_mixed": run_mixed, "loop_of_jpeg_decode": run_loop, "sorted_groups_jpeg_decode_batch": run_sorted}
    wall = {k: [] for k in calls}
    for _ in range(max(2, args.steps // 3)):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    return {"files": n, "distinct": len(distinct), "groups": len(groups), "threads": args.threads,
            "coef_MB": round(sum(2 * lay.infos[i].coef_count for i in range(n)) / 1e6, 1), "pixel_MB": round(lay.total_bytes / 1e6, 1),
            "mixed_chunks": st.chunks, "wall_ms": {k: round(v, 2) for k, v in med.items()},
            "files_per_s": {k: round(n / (v * 1e-3)) for k, v in med.items()},
            "loop_over_mixed": round(med["loop_of_jpeg_decode"] / med["batch_mixed"], 3),
            "sorted_over_mixed": round(med["sorted_groups_jpeg_decode_batch"] / med["batch_mixed"], 3), "verified": bool(ok)}


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
