#!/usr/bin/env python3
"""k_decode_scaled (csrc/hvc_scaled.hip) measured against the full-size block stage, everything in one process: the
headline's resident batch (`--frames` 1080p 4:2:0 coefficient records, config 2's frames), device events around the
dominant kernel of every call (the profiling ring), warmed, the compared calls alternating.  Every output is checked by
hvc_checksum_records against the numpy definition (tools/scaled_reference.py).  Sections (--sections, default all):

  kernel   hvc_decode_frames_scaled at scale_denom 2, 4, 8 against hvc_decode_frames: ms, the byte model's bytes
           (s = 2, 4: 128 B read + N * N B written per block; s = 8 reading the records: one 32-byte sector per block),
           what that is in TB/s, and the ratio to the full decode of the same batch
  files    the compact DC array: hvc_jpeg_decode_batch_scaled behind the GPU Huffman reader at scale_denom 8, `--files` 1080p
           files, device output, with the array (the instantiation that reads 2 B per block and no record) and without it
           (hvc_set_decode_kernel(1): the reader puts the DC into the records, k_decode_scaled reads it there), against the
           same pipeline at full size: wall time, the pipeline's own sum of reader + block stage time, and -- from the
           profiling ring, which a scaled chunk's block stage takes an entry of -- k_decode_scaled's own time summed over
           the chunks (it runs while the reader works on the next chunk: a time under that load, not of an idle GPU).
           The run counts only if the GPU reader took every chunk (entropy_ms_sum == 0).

Prints one JSON line.
    python tools/bench_scaled.py [--sections kernel,files] [--frames 1024] [--files 1024] [--steps 10] [--threads 16]
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
import scaled_reference as ref  # noqa: E402
from bench_rgb import PEAK, checksum  # noqa: E402

PLANES = [(240, 136, 0), (120, 68, 1), (120, 68, 1)]   # 1920 x 1080 4:2:0
BLOCKS = sum(bw * bh for bw, bh, _ in PLANES)


def scaled_specs(specs, n):
    out, at = [], 0
    for s in specs:
        out.append(dict(s, plane_offset=at, stride=s["blocks_w"] * n))
        at += s["blocks_w"] * n * s["blocks_h"] * n
    return out, at


def section_kernel(args, hvc, torch, ctx):
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
    calls = {"decode_frames": lambda: ctx.decode_frames(d_coefs, cfs, qtabs, comps, n, d_pix, pfs)}
    out, sspecs = {}, {}
    for s in (2, 4, 8):
        sspecs[s], fs = scaled_specs(specs, 8 // s)
        out[s] = torch.zeros((n, fs), dtype=torch.uint8, device="cuda")
        calls["scaled_%d" % s] = (lambda s=s: ctx.decode_frames_scaled(d_coefs, cfs, qtabs, sspecs[s], n, s, out[s], out[s].shape[1]))
    ctx.set_profiling(True)
    ms = {k: [] for k in calls}
    for step in range(2 + args.steps):
        for k, fn in calls.items():
            fn()
            t = ctx.last_kernel_ms()
            if step >= 2:
                ms[k].append(t)
    ctx.set_profiling(False)
    ms = {k: float(np.median(v)) for k, v in ms.items()}
    host = d_distinct.cpu().numpy()
    ok, wide = True, {}
    for s in (2, 4, 8):
        calls["scaled_%d" % s]()
        wide[s] = ctx.last_wide_blocks()
        got = ctx.checksum_records(out[s], out[s].shape[1], n)
        want = checksum([np.concatenate([ref.scaled_plane(host[f, p["coef_offset"]:p["coef_offset"] + p["blocks_w"] * p["blocks_h"] * 64],
                                                          qtabs[p["qtab"]], p["blocks_w"], p["blocks_h"], 8 // s).reshape(-1) for p in sspecs[s]])
                         for f in range(D)])
        ok &= all(got[f] == want[f % D] for f in range(n))
    model = {"decode_frames": 192, "scaled_2": 128 + 16, "scaled_4": 128 + 4, "scaled_8": 32 + 1}   # bytes per block
    res = {"frames": n, "blocks_per_frame": BLOCKS, "int64_branch_blocks": wide, "verified": bool(ok)}
    for k, v in ms.items():
        nbytes = n * BLOCKS * model[k]
        res[k] = {"ms": round(v, 4), "byte_model_bytes_per_block": model[k], "TBps": round(nbytes / (v * 1e-3) / 1e12, 3),
                  "of_8TBps_peak": round(nbytes / (v * 1e-3) / PEAK, 4), "over_decode_frames": round(v / ms["decode_frames"], 3)}
    return res


def section_files(args, hvc, torch, ctx):
    from bench_configs import config3_files
    n, D = args.files, 4
    jpegs = config3_files(ctx, D)
    batch = [jpegs[i % D] for i in range(n)]
    info = hvc.hvc.jpeg_read_header(jpegs[0])
    sinfo = hvc.hvc.jpeg_scaled_info(info, 8)
    blocks = info.coef_count // 64
    d_full = torch.zeros((n, info.pixel_bytes), dtype=torch.uint8, device="cuda")
    d_s8 = torch.zeros((n, sinfo.pixel_bytes), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def scaled_8(b, dc_array):
        # hvc_set_decode_kernel(1) makes the reader put the DC into the records (no compact array); k_decode_scaled is the same
        ctx.set_decode_kernel(0 if dc_array else 1)
        try:
            return ctx.jpeg_decode_batch_scaled(b, 8, d_s8, sinfo.pixel_bytes, threads=args.threads, gpu_entropy=True)
        finally:
            ctx.set_decode_kernel(0)

    calls = {"full": lambda b: ctx.jpeg_decode_batch_scaled(b, 1, d_full, info.pixel_bytes, threads=args.threads, gpu_entropy=True),
             "scaled_8_dc_array": lambda b: scaled_8(b, True), "scaled_8_dc_in_records": lambda b: scaled_8(b, False)}
    wall, gpu, kern = {k: [] for k in calls}, {k: [] for k in calls}, {k: [] for k in calls}
    ok = True
    for fn in calls.values():
        fn(batch[:256])   # warm-up: rings and scratch
    ctx.set_profiling(True)   # a scaled chunk's block stage takes a ring entry: k_decode_scaled alone, per chunk
    for _ in range(max(2, args.steps // 3)):
        for k, fn in calls.items():
            ctx.set_profiling(True)   # (starts the count of entries over)
            t0 = time.perf_counter()
            st = fn(batch)
            ctx.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            gpu[k].append(st.kernel_ms_sum)
            ok &= st.entropy_ms_sum == 0   # the GPU reader took every chunk: nothing went to the host reader
            if k != "full":
                kern[k].append(float(np.sum(ctx.kernel_ms_history(st.chunks))))
    ctx.set_profiling(False)
    scaled_8(batch, True)
    got = ctx.checksum_records(d_s8, sinfo.pixel_bytes, n)
    want = checksum([ctx.jpeg_decode_scaled(jpegs[f], 8)[1] for f in range(D)])
    ok &= all(got[f] == want[f % D] for f in range(n))
    med = lambda d: {k: round(float(np.median(v)), 4) for k, v in d.items() if v}
    res = {"files": n, "blocks_per_file": blocks, "wall_ms": med(wall), "reader_plus_block_stage_ms_sum": med(gpu),
           "k_decode_scaled_ms_sum_over_chunks": med(kern), "byte_model_bytes_per_block": {"scaled_8_dc_array": 2 + 1, "scaled_8_dc_in_records": 32 + 1},
           "verified": bool(ok)}
    res["model_TBps"] = {k: round(n * blocks * res["byte_model_bytes_per_block"][k] / (v * 1e-3) / 1e12, 4)
                         for k, v in res["k_decode_scaled_ms_sum_over_chunks"].items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="kernel,files")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    sections = {"kernel": section_kernel, "files": section_files}
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
