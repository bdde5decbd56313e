#!/usr/bin/env python3
"""The mixed GPU Huffman coder (csrc/hvc_huff_mixed.hip, hvc_capi_mixed_coder.hip) measured against the host coder, everything
in one process, the compared calls alternating, every file verified first.  The yardstick is hvc_jpeg_encode_batch_mixed in
the same process.

  (a) the seeded set of tools/bench_mixed_encode.py (b) -- `--files` raw frames, `--distinct` different ones repeated -- through
      hvc_jpeg_encode_batch_mixed and hvc_jpeg_encode_batch_mixed_gpu, alternating, `--runs` runs each: wall time, medians and
      minima; every file of the GPU coder's call compared with the host coder's
  (b) the same with optimised tables
  (c) the coder alone (hvc_huffman_encode_frames_mixed, device memory) on the resident records of the first `--coder-files`
      frames: device events around the call, and its wall time (the call blocks: plan, launches, offsets and status words down)
  (d) entropy_ms_sum and host_prep_ms_sum of both entry points (medians over the runs), and who coded the files

Prints one JSON line.
    python tools/bench_mixed_coder.py [--files 4096] [--distinct 256] [--runs 5] [--threads 16] [--coder-files 1024]
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

from bench_mixed_encode import mixed_frame_set  # noqa: E402


def files_section(args, ctx, frames, lay, outs, tables):
    ctx.set_huffman_tables(tables)
    calls = {"host_coder": lambda: ctx.jpeg_encode_batch_mixed(frames, threads=args.threads, layout=lay, outs=outs),
             "gpu_coder": lambda: ctx.jpeg_encode_batch_mixed_gpu(frames, threads=args.threads, layout=lay, outs=outs)}
    want = calls["host_coder"]()
    got = calls["gpu_coder"]()
    split = ctx.last_mixed_coder_files()
    ok = got == want and all(r[0] == 0 for r in got)
    seg_bytes = ctx.last_batch_stats.coef_bytes
    del want, got
    wall = {k: [] for k in calls}
    ent = {k: [] for k in calls}
    prep = {k: [] for k in calls}
    for _ in range(args.runs):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            ent[k].append(ctx.last_batch_stats.entropy_ms_sum)
            prep[k].append(ctx.last_batch_stats.host_prep_ms_sum)
    ctx.set_huffman_tables("default")
    med = {k: float(np.median(v)) for k, v in wall.items()}
    return {"tables": tables, "wall_ms": {k: round(v, 2) for k, v in med.items()},
            "wall_ms_min": {k: round(float(np.min(v)), 2) for k, v in wall.items()},
            "files_per_s": {k: round(len(frames) / (v * 1e-3)) for k, v in med.items()},
            "gpu_over_host": round(med["gpu_coder"] / med["host_coder"], 3),
            "entropy_ms_sum": {k: round(float(np.median(v)), 2) for k, v in ent.items()},
            "host_prep_ms_sum": {k: round(float(np.median(v)), 2) for k, v in prep.items()},
            "gpu_files": split[0], "host_files": split[1], "segment_MB_down": round(seg_bytes / 1e6, 1), "verified": bool(ok)}


def coder_section(args, hvc, torch, ctx, frames, keys, lay):
    """the coder alone: the block stage's records of the first frames stay on the device, the coder runs over them"""
    n = min(args.coder_files, len(frames))
    sub = hvc.hvc.jpeg_encoder_mixed_layout(keys[:n])
    pixels = np.zeros(sub.pixel_total + 8, dtype=np.uint8)
    for f in range(n):
        info, src = sub.infos[f], frames[f]
        at = 0
        for i in range(3):
            sw, sh, L = info.comp[i].actual_width, info.comp[i].actual_height, info.layout[i]
            plane = src[at:at + sw * sh].reshape(sh, sw)
            base = sub.pixel_offsets[f] + L.plane_offset
            pixels[base:base + sh * L.stride].reshape(sh, L.stride)[:, :sw] = plane   # (the padded plane has sh rows at least)
            at += sw * sh
    d_pix = torch.from_numpy(pixels).cuda()
    d_coef = torch.zeros(sub.coef_total + 8, dtype=torch.int16, device="cuda")
    po, co = list(sub.pixel_offsets)[:n], list(sub.coef_offsets)[:n]
    ctx.encode_frames_mixed(d_pix, po, sub.infos, d_coef, co)
    ctx.synchronize()
    infos = [sub.infos[f] for f in range(n)]
    out = torch.empty(2 * sub.coef_total + 4096, dtype=torch.uint8, device="cuda")
    res = {}
    ok = True
    for tables in ("default", "optimised"):
        opt = tables == "optimised"
        segs, status, _ = ctx.huffman_encode_frames_mixed(infos, d_coef, co, optimised=opt, out=out, out_cap=out.numel())
        ok &= status == [0] * n
        ev, wall = [], []
        for _ in range(2 + args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            ctx.huffman_encode_frames_mixed(infos, d_coef, co, optimised=opt, out=out, out_cap=out.numel())
            e1.record()
            e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        ev, wall = ev[2:], wall[2:]
        blocks = sub.coef_total // 64
        res[tables] = {"event_ms": round(float(np.median(ev)), 3), "event_ms_min": round(float(np.min(ev)), 3),
                       "wall_ms": round(float(np.median(wall)), 3), "segment_MB": round(sum(len(s) for s in segs) / 1e6, 1),
                       "Gblocks_per_s_by_events": round(blocks / (float(np.median(ev)) * 1e-3) / 1e9, 3)}
    res.update({"files": n, "coef_MB": round(2 * sub.coef_total / 1e6, 1), "verified": bool(ok)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    ap.add_argument("--coder-files", dest="coder_files", type=int, default=1024)
    ap.add_argument("--sections", default="default,optimised,coder")
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    distinct, dkeys = mixed_frame_set(min(args.distinct, args.files))
    D = len(distinct)
    frames = [distinct[i % D] for i in range(args.files)]
    keys = [dkeys[i % D] for i in range(args.files)]
    lay = hvc.hvc.jpeg_encoder_mixed_layout(keys)
    outs = [np.empty(4 * w * h + 65536, dtype=np.uint8) for w, h, _, _ in keys]
    res = {"kernel_id": hvc.hvc.kernel_build_id(), "files": args.files, "distinct": D, "threads": args.threads, "runs": args.runs,
           "pixel_MB": round(lay.pixel_total / 1e6, 1), "coef_MB": round(2 * lay.coef_total / 1e6, 1)}
    ctx = hvc.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ok = True
    try:
        for name in [s for s in args.sections.split(",") if s]:
            if name == "coder":
                res["coder_alone"] = coder_section(args, hvc, torch, ctx, frames, keys, lay)
                ok &= res["coder_alone"]["verified"]
            else:
                res[name] = files_section(args, ctx, frames, lay, outs, name)
                ok &= res[name]["verified"]
    finally:
        ctx.close()
    res["verified"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
