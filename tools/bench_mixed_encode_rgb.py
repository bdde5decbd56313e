#!/usr/bin/env python3
"""Mixed encode batches from RGB images (k_rgb_to_ycc_mixed, csrc/hvc_mixed_rgb.hip; hvc_capi_mixed_encode.hip) measured against
the single-geometry entry points, everything in one process, the compared calls alternating, every output verified first,
medians of `--steps` (5).  Sections (--sections):

  kernel  (a) hvc_rgb_to_yuv_mixed on `--frames` (1024) 1080p 4:2:0 images, HBM-resident, against hvc_rgb_to_yuv on the same
          images: device events around the call on the stream both run on (k_rgb_to_ycc_mixed / k_rgb_to_ycc are the only
          kernels between them; the mixed call's tables are on the device after the first call), and, for the mixed call, the
          profiling ring's pair around the kernel alone (the host builds the plan between the first event and the launch).
          Same bytes moved plus 4 bytes of work map per 64 lanes and a descriptor per image.
  files   (b) the seeded set of tools/bench_mixed_encode.py -- `--files` (4096) frames, even sides 64 .. 1024, 4:2:0 / 4:2:2 /
          4:4:4, qualities 20 / 50 / 75 / 95, `--distinct` different ones repeated -- as RGB images, through
          hvc_jpeg_encode_batch_mixed_rgb and _rgb_gpu, against a loop of hvc_jpeg_encode_rgb and against hvc_rgb_to_yuv per
          image followed by hvc_jpeg_encode_batch_mixed[_gpu]: wall time.
  stages  (c) one chunk's worth of that set (64 MiB of padded pixel records) on device memory: clearing the plane slot (a
          device fill of the same bytes, standing in for the pipeline's hipMemsetAsync; events around it), k_rgb_to_ycc_mixed
          and k_encode_mixed (the profiling ring's pair around each kernel) -> the clear's and the colour pass's share of the
          three.

Prints one JSON line.
    python tools/bench_mixed_encode_rgb.py [--sections kernel,files,stages] [--frames 1024] [--files 4096] [--distinct 256] [--steps 5] [--threads 16]
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


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def section_kernel(args, hvc, torch, ctx):
    n, w, h, D = args.frames, 1920, 1080, 4
    info = hvc.hvc.jpeg_encoder_layout(w, h, 420, 75)
    comps = info.layout
    src = torch.randint(0, 256, (D, h, w, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    d_rgb = src.repeat((n + D - 1) // D, 1, 1, 1)[:n].contiguous()
    fs = (info.pixel_bytes + 63) & ~63
    d_one = torch.zeros((n, fs), dtype=torch.uint8, device="cuda")
    d_mix = torch.zeros((n, fs), dtype=torch.uint8, device="cuda")
    infos = (hvc.hvc.JpegInfo * n)(*([info] * n))
    yo = (C.c_size_t * n)(*[f * fs for f in range(n)])
    ro = (C.c_size_t * n)(*[f * 3 * w * h for f in range(n)])
    calls = {"rgb_to_yuv": lambda: ctx.rgb_to_yuv(d_rgb, w, h, 420, d_one, comps, n_frames=n, yuv_frame_stride=fs),
             "rgb_to_yuv_mixed": lambda: ctx.rgb_to_yuv_mixed(d_mix, yo, infos, d_rgb, ro)}
    for fn in calls.values():
        fn()
    ctx.synchronize()
    ok = bool(torch.equal(d_one, d_mix)) and bool(d_mix.any())
    # events around each call on the stream both run on; the mixed call also by the profiling ring, whose pair brackets the
    # kernel alone: the events around it see the host build and compare its plan (a map entry per 64 lanes) before the launch
    ctx.set_profiling(True)
    ms = {k: [] for k in list(calls) + ["k_rgb_to_ycc_mixed_alone"]}
    for step in range(2 + args.steps):
        for k, fn in calls.items():
            t = event_ms(torch, fn)
            if step >= 2:
                ms[k].append(t)
                if k == "rgb_to_yuv_mixed":
                    ms["k_rgb_to_ycc_mixed_alone"].append(ctx.last_kernel_ms())
    ctx.set_profiling(False)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    moved = n * (3 * w * h + w * h + 2 * (w // 2) * (h // 2))   # RGB read, the frame's own samples written
    return {"frames": n, "size": "%dx%d 4:2:0" % (w, h), "work_units": n * (-(-(w // 8) * (h // 2) // 64)),
            "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
            "TBps": {k: round(moved / (v * 1e-3) / 1e12, 3) for k, v in med.items()},
            "mixed_over_rgb_to_yuv": round(med["rgb_to_yuv_mixed"] / med["rgb_to_yuv"], 4),
            "mixed_kernel_alone_over_rgb_to_yuv": round(med["k_rgb_to_ycc_mixed_alone"] / med["rgb_to_yuv"], 4), "verified": ok}


def rgb_frame_set(distinct):
    """the (width, height, chroma, quality) draws of tools/bench_mixed_encode.py's seeded set, each with an RGB image [h, w, 3]:
    smooth content with noise, a different phase per channel"""
    from bench_mixed_encode import mixed_frame_set
    _, keys = mixed_frame_set(distinct)
    rng = np.random.Generator(np.random.PCG64(20261019))
    images = []
    for w, h, _, _ in keys:
        yy, xx = np.mgrid[0:h, 0:w]
        ch = [128 + 90 * np.sin(xx / float(rng.integers(5, 60)) + yy / float(rng.integers(5, 60)) + k) + rng.integers(-12, 13, size=(h, w))
              for k in range(3)]
        images.append(np.ascontiguousarray(np.clip(np.stack(ch, axis=2), 0, 255).astype(np.uint8)))
    return images, keys


def section_files(args, hvc, torch, ctx):
    n = args.files
    distinct, dkeys = rgb_frame_set(min(args.distinct, n))
    D = len(distinct)
    images = [distinct[i % D] for i in range(n)]
    keys = [dkeys[i % D] for i in range(n)]
    lay = hvc.hvc.jpeg_encoder_mixed_rgb_layout(keys)
    yuv_lay = hvc.hvc.jpeg_encoder_mixed_layout(keys)
    outs = [np.empty(4 * w * h + 65536, dtype=np.uint8) for w, h, _, _ in keys]

    def to_yuv(i):
        w, h, chroma, _ = keys[i]
        info = lay.infos[i]
        rec = np.zeros(info.pixel_bytes, dtype=np.uint8)
        ctx.rgb_to_yuv(images[i], w, h, chroma, rec, info.layout)
        out = []
        for k in range(3):   # the frame's own samples out of the padded record: tight Y, U, V
            L, aw, ah = info.layout[k], info.comp[k].actual_width, info.comp[k].actual_height
            out.append(rec[L.plane_offset:L.plane_offset + L.stride * ah].reshape(ah, L.stride)[:, :aw].reshape(-1))
        return np.concatenate(out)

    def run_rgb(coder):
        return ctx.jpeg_encode_batch_mixed_rgb(images, threads=args.threads, enc_layout=lay, outs=outs, coder=coder)

    def run_loop():
        return [ctx.jpeg_encode_rgb(images[i], keys[i][2], keys[i][3]) for i in range(n)]

    def run_convert_then_yuv(coder):
        return ctx.jpeg_encode_batch_mixed([to_yuv(i) for i in range(n)], threads=args.threads, layout=yuv_lay, outs=outs, coder=coder)

    # verification first: every file of every path == hvc_jpeg_encode_rgb's for that image
    single = [ctx.jpeg_encode_rgb(distinct[i], dkeys[i][2], dkeys[i][3]) for i in range(D)]
    ok, stats = True, {}
    for coder in ("host", "gpu"):
        res = run_rgb(coder)
        st = ctx.last_batch_stats
        stats[coder] = {"wall_ms": round(st.wall_ms, 2), "entropy_ms_sum": round(st.entropy_ms_sum, 2), "host_prep_ms_sum": round(st.host_prep_ms_sum, 2),
                        "h2d_ms_sum": round(st.h2d_ms_sum, 2), "kernel_ms_sum": round(st.kernel_ms_sum, 2), "d2h_ms_sum": round(st.d2h_ms_sum, 2),
                        "chunks": st.chunks}
        ok &= all(r[0] == 0 and r[1] == single[i % D] for i, r in enumerate(res))
    ok &= all(r[0] == 0 and r[1] == single[i % D] for i, r in enumerate(run_convert_then_yuv("host")))
    calls = {"batch_mixed_rgb": lambda: run_rgb("host"), "batch_mixed_rgb_gpu": lambda: run_rgb("gpu"),
             "loop_of_jpeg_encode_rgb": run_loop, "rgb_to_yuv_each_then_batch_mixed": lambda: run_convert_then_yuv("host"),
             "rgb_to_yuv_each_then_batch_mixed_gpu": lambda: run_convert_then_yuv("gpu")}
    wall = {k: [] for k in calls}
    for _ in range(args.steps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    return {"files": n, "distinct": D, "threads": args.threads, "rgb_MB": round(lay.rgb_total / 1e6, 1), "pixel_MB": round(lay.pixel_total / 1e6, 1),
            "jpeg_MB": round(sum(len(s) for s in single) * (n / D) / 1e6, 1), "first_call_stats": stats,
            "wall_ms": {k: round(v, 2) for k, v in med.items()}, "wall_ms_min": {k: round(float(np.min(v)), 2) for k, v in wall.items()},
            "files_per_s": {k: round(n / (v * 1e-3)) for k, v in med.items()},
            "loop_over_mixed_rgb": round(med["loop_of_jpeg_encode_rgb"] / med["batch_mixed_rgb"], 3),
            "loop_over_mixed_rgb_gpu": round(med["loop_of_jpeg_encode_rgb"] / med["batch_mixed_rgb_gpu"], 3),
            "convert_then_yuv_over_mixed_rgb": round(med["rgb_to_yuv_each_then_batch_mixed"] / med["batch_mixed_rgb"], 3),
            "convert_then_yuv_gpu_over_mixed_rgb_gpu": round(med["rgb_to_yuv_each_then_batch_mixed_gpu"] / med["batch_mixed_rgb_gpu"], 3),
            "verified": bool(ok)}


def section_stages(args, hvc, torch, ctx):
    distinct, dkeys = rgb_frame_set(min(args.distinct, args.files))
    keys, images, total = [], [], 0
    for i in range(args.files):                                       # the first chunk the pipeline would cut: 64 MiB of records
        info = hvc.hvc.jpeg_encoder_layout(*dkeys[i % len(dkeys)])
        if total + ((info.pixel_bytes + 63) & ~63) > (64 << 20):
            break
        total += (info.pixel_bytes + 63) & ~63
        keys.append(dkeys[i % len(dkeys)])
        images.append(distinct[i % len(dkeys)])
    lay = hvc.hvc.jpeg_encoder_mixed_rgb_layout(keys)
    n = len(keys)
    rgb = np.zeros(lay.rgb_total + 8, dtype=np.uint8)
    for f, im in enumerate(images):
        rgb[lay.rgb_offsets[f]:lay.rgb_offsets[f] + im.size] = im.reshape(-1)
    d_rgb = torch.from_numpy(rgb).cuda()
    d_planes = torch.zeros(lay.pixel_total + 64, dtype=torch.uint8, device="cuda")
    d_coefs = torch.zeros(lay.coef_total + 64, dtype=torch.int16, device="cuda")
    d_fused = torch.zeros(lay.coef_total + 64, dtype=torch.int16, device="cuda")
    calls = {"clear_plane_slot": lambda: d_planes.zero_(),
             "k_rgb_to_ycc_mixed": lambda: ctx.rgb_to_yuv_mixed(d_planes, lay.pixel_offsets, lay.infos, d_rgb, lay.rgb_offsets),
             "k_encode_mixed": lambda: ctx.encode_frames_mixed(d_planes, lay.pixel_offsets, lay.infos, d_coefs, lay.coef_offsets)}
    for fn in calls.values():
        fn()
    ctx.encode_frames_mixed_rgb(d_rgb, lay.rgb_offsets, lay.infos, d_fused, lay.coef_offsets)
    ctx.synchronize()
    ok = bool(torch.equal(d_coefs, d_fused)) and bool(d_coefs.any())
    ctx.set_profiling(True)   # the two kernels by the profiling ring (the pair brackets the kernel alone), the fill by events around it
    ms = {k: [] for k in calls}
    for step in range(2 + args.steps):
        for k, fn in calls.items():
            t = event_ms(torch, fn)
            if step >= 2:
                ms[k].append(t if k == "clear_plane_slot" else ctx.last_kernel_ms())
    ctx.set_profiling(False)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    tot = sum(med.values())
    return {"frames": n, "pixel_MB": round(lay.pixel_total / 1e6, 1), "rgb_MB": round(lay.rgb_total / 1e6, 1),
            "ms": {k: round(v, 4) for k, v in med.items()}, "share": {k: round(v / tot, 3) for k, v in med.items()}, "verified": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="kernel,files,stages")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    sections = {"kernel": section_kernel, "files": section_files, "stages": section_stages}
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
        print(json.dumps({name: res[name]}), file=sys.stderr, flush=True)
    res["verified"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
