#!/usr/bin/env python3
"""The RGB colour pass (csrc/hvc_rgb.hip) measured, everything in one process, device events on the context's stream,
warmed, the compared calls alternating; every output is checked by hvc_checksum_records against the numpy definition
(tools/rgb_reference.py) on sampled frames.  Sections (--sections, default all):

  kernel   k_ycc_to_rgb alone on `--frames` 1080p 4:2:0 resident planes, both layouts: ms, algorithmic bytes
           (w * h * 4.5 per frame), TB/s, share of the 8 TB/s peak and of the 6.29 TB/s copy rate; the yardstick in the
           same process is hvc_upsample420 on the same chroma planes (1 B read + 4 B written per chroma sample)
  decode   hvc_decode_frames_rgb against hvc_decode_frames_yuv444 and hvc_decode_frames on config 2's batch
           (byte model 9 : 6 : 4.5 bytes per pixel)
  files    hvc_jpeg_decode_batch_rgb (GPU reader, device output) against hvc_jpeg_decode_batch_gpu with yuv444 on
           `--files` 1080p files (config 3's)
  encode   k_rgb_to_ycc alone on config 5's frames (`--frames-4k` 4K images -> 4:2:0 planes), and hvc_jpeg_encode_rgb
           against hvc_jpeg_encode of the same frame (the conversion's share of one file)

Prints one JSON line.
    python tools/bench_rgb.py [--sections kernel,decode,files,encode] [--frames 1024] [--files 4096] [--frames-4k 256]
                              [--steps 10] [--threads 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rgb_reference as ref  # noqa: E402

PEAK, COPY = 8e12, 6.29e12   # HBM peak and the measured copy rate of an MI355X, bytes per second
CHECKSUM_MUL = np.uint64(0x9E3779B97F4A7C15)


def checksum(records):
    """hvc_checksum_records in numpy: uint8 [n][bytes] -> uint64 [n]"""
    records = np.ascontiguousarray(records, dtype=np.uint8).reshape(len(records), -1)
    with np.errstate(over="ignore"):
        w = (np.arange(records.shape[1], dtype=np.uint64) * np.uint64(2) + np.uint64(1)) * CHECKSUM_MUL
        return ((records.astype(np.uint64) + np.uint64(1)) * w[None, :]).sum(axis=1, dtype=np.uint64)


def timed(ctx, calls, steps, warmup=2):
    """{name: fn} -> {name: median ms}, the calls alternating, each between device events on the context's stream"""
    ms = {k: [] for k in calls}
    for step in range(warmup + steps):
        for k, fn in calls.items():
            ctx.timer_begin()
            fn()
            t = ctx.timer_end()
            if step >= warmup:
                ms[k].append(t)
    return {k: float(np.median(v)) for k, v in ms.items()}


def planes_of_record(rec, specs, width_of=lambda s: s["blocks_w"] * 8):
    return [rec[s["plane_offset"]:s["plane_offset"] + s["blocks_w"] * s["blocks_h"] * 64].reshape(-1, width_of(s)) for s in specs]


def rate(nbytes, ms):
    bps = nbytes / (ms * 1e-3)
    return {"ms": round(ms, 4), "TBps": round(bps / 1e12, 3), "of_8TBps_peak": round(bps / PEAK, 4), "of_6.29TBps_copy": round(bps / COPY, 4)}


def section_kernel(args, hvc, torch, ctx):
    W, H, n, D = 1920, 1080, args.frames, 4
    planes = [(240, 136, 0), (120, 68, 1), (120, 68, 1)]
    specs, _, pfs = hvc.hvc.frame_layout(planes)
    rng = np.random.Generator(np.random.PCG64(11))
    distinct = rng.integers(0, 256, size=(D, pfs), dtype=np.uint8)
    d_yuv = torch.from_numpy(distinct).cuda().repeat((n + D - 1) // D, 1)[:n].contiguous()
    d_rgb = torch.zeros((n, 3 * W * H), dtype=torch.uint8, device="cuda")
    d_up = torch.zeros((2 * n, W * H), dtype=torch.uint8, device="cuda")

    def upsample():  # the two chroma planes of every frame: 960 x 540 windows of the 960 x 544 planes
        for k in (1, 2):
            ctx.upsample420(d_yuv[:, specs[k]["plane_offset"]:], W // 2, H // 2, d_up[(k - 1) * n:], n_planes=n, src_stride=960,
                            dst_stride=W, src_plane_stride=pfs, dst_plane_stride=W * H)

    calls = {"interleaved": lambda: ctx.yuv_to_rgb(d_yuv, specs, 420, W, H, d_rgb, n_frames=n, yuv_frame_stride=pfs),
             "planar": lambda: ctx.yuv_to_rgb(d_yuv, specs, 420, W, H, d_rgb, n_frames=n, yuv_frame_stride=pfs, layout="planar"),
             "upsample420": upsample}
    ms = timed(ctx, calls, args.steps)
    ok = True
    for layout in ("interleaved", "planar"):
        calls[layout]()
        sample = [0, 1, 2, 3, n - 1]
        got = ctx.checksum_records(d_rgb, 3 * W * H, n)
        want = checksum([ref.planes_to_rgb(*planes_of_record(distinct[f % D], specs), 420, W, H, layout) for f in sample])
        ok &= all(got[f] == want[i] for i, f in enumerate(sample))
        ok &= all(got[f] == got[f % D] for f in range(n))
    algo = n * W * H * 4.5
    return {"frames": n, "geometry": "1920x1080 4:2:0 planes of the decoder's record -> RGB", "algorithmic_bytes": int(algo),
            "k_ycc_to_rgb_interleaved": rate(algo, ms["interleaved"]), "k_ycc_to_rgb_planar": rate(algo, ms["planar"]),
            "hvc_upsample420_same_chroma_planes": rate(2 * n * (W // 2) * (H // 2) * 5, ms["upsample420"]), "verified": bool(ok)}


def section_decode(args, hvc, torch, ctx):
    from video_coding_amd.synth import synth_frame_pixels
    W, H, n, D = 1920, 1080, args.frames, 4
    planes = [(240, 136, 0), (120, 68, 1), (120, 68, 1)]
    qtabs = np.stack([hvc.hvc.quant_table(0, 75), hvc.hvc.quant_table(1, 75)])
    specs, cfs, pfs = hvc.hvc.frame_layout(planes)
    comps = hvc.hvc.components(specs)
    src = torch.from_numpy(np.stack([synth_frame_pixels(40 + 8 * f, planes) for f in range(D)])).cuda()   # config 2's frames
    d_distinct = torch.zeros((D, cfs), dtype=torch.int16, device="cuda")
    ctx.encode_frames(src, pfs, qtabs, comps, D, d_distinct, cfs)
    d_coefs = d_distinct.repeat((n + D - 1) // D, 1)[:n].contiguous()
    d_out = torch.zeros((n, 3 * W * H), dtype=torch.uint8, device="cuda")
    d_pix = torch.zeros((n, pfs), dtype=torch.uint8, device="cuda")
    calls = {"decode_frames_rgb": lambda: ctx.decode_frames_rgb(d_coefs, cfs, qtabs, comps, 420, n, W, H, d_out),
             "decode_frames_yuv444": lambda: ctx.decode_frames_yuv444(d_coefs, cfs, qtabs, comps, n, W, H, d_out),
             "decode_frames": lambda: ctx.decode_frames(d_coefs, cfs, qtabs, comps, n, d_pix, pfs)}
    ms = timed(ctx, calls, args.steps)
    calls["decode_frames"]()
    calls["decode_frames_rgb"]()
    ctx.synchronize()
    host_planes = d_pix[:D].cpu().numpy()   # (hvc_decode_frames' planes: what bench.py verifies against the model)
    got = ctx.checksum_records(d_out, 3 * W * H, n)
    want = checksum([ref.planes_to_rgb(*planes_of_record(host_planes[f], specs), 420, W, H) for f in range(D)])
    ok = all(got[f] == want[f % D] for f in range(n))
    px = n * W * H
    return {"frames": n, "ms": {k: round(v, 4) for k, v in ms.items()},
            "Gpixel_s": {k: round(px / (v * 1e-3) / 1e9, 2) for k, v in ms.items()},
            "byte_model_bytes_per_pixel": {"decode_frames_rgb": 9, "decode_frames_yuv444": 6, "decode_frames": 4.5},
            "measured_ratio_over_decode_frames": {k: round(v / ms["decode_frames"], 3) for k, v in ms.items()},
            "verified": bool(ok)}


def section_files(args, hvc, torch, ctx):
    from bench_configs import config3_files
    W, H, n, D = 1920, 1080, args.files, 4
    jpegs = config3_files(ctx, D)
    batch = [jpegs[i % D] for i in range(n)]
    d_out = torch.zeros((n, 3 * W * H), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    calls = {"jpeg_decode_batch_rgb": lambda b: ctx.jpeg_decode_batch_rgb(b, d_out, threads=args.threads, gpu_entropy=True),
             "jpeg_decode_batch_gpu_yuv444": lambda b: ctx.jpeg_decode_batch(b, d_out, 3 * W * H, threads=args.threads, frames_per_chunk=0,
                                                                             yuv444=True, gpu_entropy=True)}
    wall = {k: [] for k in calls}
    for k, fn in calls.items():
        fn(batch[:256])   # warm-up: rings and scratch
    for _ in range(max(2, args.steps // 3)):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn(batch)
            ctx.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    calls["jpeg_decode_batch_rgb"](batch)
    ctx.synchronize()
    got = ctx.checksum_records(d_out, 3 * W * H, n)
    want = []
    for f in range(D):
        info, pixels = ctx.jpeg_decode(jpegs[f])
        want.append(ref.planes_to_rgb(*info.planes(pixels), 420, W, H))
    want = checksum(want)
    ok = all(got[f] == want[f % D] for f in range(n))
    med = {k: float(np.median(v)) for k, v in wall.items()}
    return {"files": n, "wall_ms": {k: round(v, 2) for k, v in med.items()},
            "Gpixel_s": {k: round(n * W * H / (v * 1e-3) / 1e9, 2) for k, v in med.items()},
            "rgb_over_yuv444": round(med["jpeg_decode_batch_rgb"] / med["jpeg_decode_batch_gpu_yuv444"], 3), "verified": bool(ok)}


def section_encode(args, hvc, torch, ctx):
    from video_coding_amd.synth import synth_pixels
    W, H, n, D = 3840, 2160, args.frames_4k, 4
    images = np.stack([np.stack([synth_pixels(110 + 10 * k + f, H, W) for k in range(3)], axis=2) for f in range(D)])
    d_rgb = torch.from_numpy(images).cuda().repeat((n + D - 1) // D, 1, 1, 1)[:n].contiguous()
    info = hvc.hvc.jpeg_encoder_layout(W, H, 420, 75)
    specs = [dict(blocks_w=L.blocks_w, blocks_h=L.blocks_h, plane_offset=L.plane_offset, stride=L.stride) for L in info.layout[:3]]
    pfs = info.pixel_bytes
    d_yuv = torch.zeros((n, pfs), dtype=torch.uint8, device="cuda")
    calls = {"interleaved": lambda: ctx.rgb_to_yuv(d_rgb, W, H, 420, d_yuv, specs, n_frames=n, yuv_frame_stride=pfs)}
    ms = timed(ctx, calls, args.steps)
    calls["interleaved"]()
    got = ctx.checksum_records(d_yuv, pfs, n)
    want = []
    for f in range(D):
        y, u, v = ref.rgb_to_planes(images[f], 420)
        want.append(hvc.hvc.encoder_pixel_record(info, y, u, v, W, H, 420))
    want = checksum(want)
    ok = all(got[f] == want[f % D] for f in range(n))
    # one file: hvc_jpeg_encode_rgb against hvc_jpeg_encode of the converted planes (wall time, host image in, file out)
    y, u, v = ref.rgb_to_planes(images[0], 420)
    one = {"jpeg_encode_rgb": lambda: ctx.jpeg_encode_rgb(images[0], 420, 75), "jpeg_encode": lambda: ctx.jpeg_encode(y, u, v, W, H, 420, 75)}
    wall, files = {k: [] for k in one}, {}
    for step in range(args.steps + 1):
        for k, fn in one.items():
            t0 = time.perf_counter()
            files[k] = fn()
            if step:
                wall[k].append((time.perf_counter() - t0) * 1e3)
    ok &= files["jpeg_encode_rgb"] == files["jpeg_encode"]
    med = {k: float(np.median(v)) for k, v in wall.items()}
    algo = n * W * H * 4.5
    return {"frames": n, "geometry": "3840x2160 RGB -> 4:2:0 planes of the encoder's record", "algorithmic_bytes": int(algo),
            "k_rgb_to_ycc_interleaved": rate(algo, ms["interleaved"]),
            "one_4k_file_wall_ms": {k: round(v, 2) for k, v in med.items()},
            "conversion_kernel_ms_per_frame": round(ms["interleaved"] / n, 4),
            "conversion_share_of_jpeg_encode_rgb": round(ms["interleaved"] / n / med["jpeg_encode_rgb"], 4), "verified": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="kernel,decode,files,encode")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--frames-4k", dest="frames_4k", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    sections = {"kernel": section_kernel, "decode": section_decode, "files": section_files, "encode": section_encode}
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
