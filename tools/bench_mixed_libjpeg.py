#!/usr/bin/env python3
"""The libjpeg-exact mixed batch (hvc_set_mixed_arithmetic HVC_ARITH_LIBJPEG; csrc/hvc_mixed_libjpeg.hip) measured against its
uniform kernels and against the model-arithmetic mixed calls: one process, the compared calls ALTERNATING, device events,
medians of `--runs`, outputs verified against the per-file calls on a sample.  Sections (--sections, default all):

  block    (a) k_islow_mixed against k_islow and against k_decode_mixed on the headline's uniform batch (`--frames` 1080p 4:2:0
           records, HBM-resident): hvc_decode_frames_mixed under both mixed settings and hvc_decode_frames under
           HVC_ARITH_LIBJPEG on the same records, the kernels' own time from the profiling ring.
  colour   (b) k_ycc_to_rgb_fancy_mixed against k_ycc_to_rgb_fancy and against k_ycc_to_rgb_mixed on that batch's planes:
           hvc_yuv_to_rgb_mixed under both settings (profiling ring) and hvc_yuv_to_rgb under HVC_ARITH_LIBJPEG (the whole call
           between device events: its launches are all there is to it).
  files    (c) the seeded `--files`-file set of tools/bench_mixed.py through hvc_jpeg_decode_batch_mixed_rgb with both settings
           alternating, and against a loop of hvc_jpeg_decode_rgb under HVC_ARITH_LIBJPEG: wall time.
  resized  (d) the same set to a 224 x 224 tensor through hvc_jpeg_decode_batch_mixed_resized under both settings: wall time.

Prints one JSON line.
    python tools/bench_mixed_libjpeg.py [--sections block,colour,files,resized] [--frames 1024] [--files 4096] [--distinct 256] [--runs 5] [--threads 16]
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
import libjpeg_reference as lj  # noqa: E402
import resize_reference as rr  # noqa: E402
from bench_mixed import BLOCKS, PLANES, mixed_file_set  # noqa: E402

W, H = 1920, 1080
SETTINGS = ("model", "libjpeg")


def med(v):
    return round(float(np.median(v)), 4)


class Uniform:
    """the headline's uniform batch as records in HBM, with the descriptors of both kinds of call"""

    def __init__(self, hvc, torch, ctx, n):
        from video_coding_amd.synth import synth_frame_pixels
        D = 4
        self.n, self.qtabs = n, np.stack([hvc.hvc.quant_table(0, 75), hvc.hvc.quant_table(1, 75)])
        self.specs, self.cfs, self.pfs = hvc.hvc.frame_layout(PLANES)
        self.comps = hvc.hvc.components(self.specs)
        src = torch.from_numpy(np.stack([synth_frame_pixels(40 + 8 * f, PLANES) for f in range(D)])).cuda()
        self.distinct = torch.zeros((D, self.cfs), dtype=torch.int16, device="cuda")
        ctx.encode_frames(src, self.pfs, self.qtabs, self.comps, D, self.distinct, self.cfs)
        self.coefs = self.distinct.repeat((n + D - 1) // D, 1)[:n].contiguous()
        info = hvc.hvc.JpegInfo()
        info.n_comp, info.n_qtabs, info.coef_count, info.pixel_bytes, info.width, info.height = len(self.specs), 2, self.cfs, self.pfs, W, H
        for t in range(2):
            for k in range(64):
                info.qtabs[t][k] = int(self.qtabs[t][k])
        for i, s in enumerate(self.specs):
            L = info.layout[i]
            L.blocks_w, L.blocks_h, L.qtab, L.coef_offset, L.plane_offset, L.stride = (s["blocks_w"], s["blocks_h"], s["qtab"], s["coef_offset"],
                                                                                       s["plane_offset"], s["stride"])
            info.comp[i].hscale, info.comp[i].vscale = (2, 2) if i == 0 else (1, 1)
        self.infos = (hvc.hvc.JpegInfo * n)(*([info] * n))
        self.co = (C.c_size_t * n)(*[f * self.cfs for f in range(n)])
        self.po = (C.c_size_t * n)(*[f * self.pfs for f in range(n)])
        self.ro = (C.c_size_t * n)(*[f * 3 * W * H for f in range(n)])


def section_block(args, hvc, torch, uni, mix, U):
    n = U.n
    d_uni = torch.zeros((n, U.pfs), dtype=torch.uint8, device="cuda")
    d_mix = torch.zeros((n, U.pfs), dtype=torch.uint8, device="cuda")

    def mixed(setting):
        mix.set_mixed_arithmetic(setting)
        mix.decode_frames_mixed(U.coefs, U.co, U.infos, d_mix, U.po)
        return mix
    calls = {"k_islow": lambda: (uni.decode_frames(U.coefs, U.cfs, U.qtabs, U.comps, n, d_uni, U.pfs), uni)[1],
             "k_decode_mixed": lambda: mixed("model"), "k_islow_mixed": lambda: mixed("libjpeg")}
    for fn in calls.values():
        fn().synchronize()
    ok = bool(torch.equal(d_uni, d_mix)) and mix.last_wide_blocks() == 0    # (the last call was k_islow_mixed's)
    host, got = U.distinct[0].cpu().numpy(), d_mix[0].cpu().numpy()
    for s, p in zip(U.specs, lj.record_planes(host, U.qtabs, PLANES)):
        ok &= bool(np.array_equal(got[s["plane_offset"]:s["plane_offset"] + p.size].reshape(p.shape), p))
    uni.set_profiling(True)
    mix.set_profiling(True)
    ms = {k: [] for k in calls}
    for run in range(2 + args.runs):
        for k, fn in calls.items():
            c = fn()
            c.synchronize()
            if run >= 2:
                ms[k].append(c.last_kernel_ms())
    uni.set_profiling(False)
    mix.set_profiling(False)
    m = {k: float(np.median(v)) for k, v in ms.items()}
    return {"frames": n, "ms": {k: med(v) for k, v in ms.items()}, "ms_min": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
            "TBps": {k: round(n * BLOCKS * 192 / (v * 1e-3) / 1e12, 3) for k, v in m.items()},
            "islow_mixed_over_islow": round(m["k_islow_mixed"] / m["k_islow"], 4),
            "islow_mixed_over_decode_mixed": round(m["k_islow_mixed"] / m["k_decode_mixed"], 4), "verified": ok}, d_mix


def section_colour(args, hvc, torch, uni, mix, U, d_planes):
    n = U.n
    d_uni = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    d_mix = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")

    def mixed(setting):
        mix.set_mixed_arithmetic(setting)
        mix.yuv_to_rgb_mixed(d_planes, U.po, U.infos, d_mix, U.ro)
    uni.yuv_to_rgb(d_planes, U.comps, 420, W, H, d_uni, n_frames=n, yuv_frame_stride=U.pfs)
    mixed("libjpeg")
    uni.synchronize()
    mix.synchronize()
    ok = bool(torch.equal(d_uni, d_mix))
    pl = d_planes[0].cpu().numpy()
    p = [pl[s["plane_offset"]:s["plane_offset"] + s["stride"] * s["blocks_h"] * 8].reshape(-1, s["stride"]) for s in U.specs]
    ok &= bool(np.array_equal(d_mix[0].cpu().numpy(), lj.planes_to_rgb(p[0], p[1], p[2], 420, W, H)))
    ms = {"k_ycc_to_rgb_fancy": [], "k_ycc_to_rgb_mixed": [], "k_ycc_to_rgb_fancy_mixed": []}
    mix.set_profiling(True)
    for run in range(2 + args.runs):
        uni.timer_begin()
        uni.yuv_to_rgb(d_planes, U.comps, 420, W, H, d_uni, n_frames=n, yuv_frame_stride=U.pfs)
        t = {"k_ycc_to_rgb_fancy": uni.timer_end()}
        for setting, k in (("model", "k_ycc_to_rgb_mixed"), ("libjpeg", "k_ycc_to_rgb_fancy_mixed")):
            mixed(setting)
            mix.synchronize()
            t[k] = mix.last_kernel_ms()
        if run >= 2:
            for k, v in t.items():
                ms[k].append(v)
    mix.set_profiling(False)
    m = {k: float(np.median(v)) for k, v in ms.items()}
    algo = int(n * W * H * 4.5)
    return {"frames": n, "ms": {k: med(v) for k, v in ms.items()}, "ms_min": {k: round(float(np.min(v)), 4) for k, v in ms.items()},
            "TBps": {k: round(algo / (v * 1e-3) / 1e12, 3) for k, v in m.items()},
            "fancy_mixed_over_fancy": round(m["k_ycc_to_rgb_fancy_mixed"] / m["k_ycc_to_rgb_fancy"], 4),
            "fancy_mixed_over_rgb_mixed": round(m["k_ycc_to_rgb_fancy_mixed"] / m["k_ycc_to_rgb_mixed"], 4), "verified": ok}


def walls(calls, runs, sync):
    wall = {k: [] for k in calls}
    for _ in range(runs):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            sync()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return wall


def section_files(args, hvc, torch, uni, mix, files, distinct):
    n = len(files)
    lay = hvc.hvc.jpeg_mixed_rgb_layout(files)
    rgb = np.zeros(lay.total_bytes, dtype=np.uint8)

    def mixed(setting):
        mix.set_mixed_arithmetic(setting)
        return mix.jpeg_decode_batch_mixed_rgb(files, threads=args.threads, rgb_layout=lay, rgb=rgb)
    res = mixed("libjpeg")
    ok = all(r[0] == 0 for r in res)
    for i in range(0, n, max(1, n // 64)):                      # a sample: the per-file call under HVC_ARITH_LIBJPEG
        ok &= bool(np.array_equal(res[i][2], uni.jpeg_decode_rgb(files[i])[1]))
    calls = {"mixed_rgb_model": lambda: mixed("model"), "mixed_rgb_libjpeg": lambda: mixed("libjpeg"),
             "loop_of_jpeg_decode_rgb_libjpeg": lambda: [uni.jpeg_decode_rgb(f) for f in files]}
    wall = walls(calls, args.runs, mix.synchronize)
    m = {k: float(np.median(v)) for k, v in wall.items()}
    return {"files": n, "distinct": distinct, "threads": args.threads, "rgb_MB": round(lay.total_bytes / 1e6, 1),
            "wall_ms": {k: round(v, 2) for k, v in m.items()}, "files_per_s": {k: round(n / (v * 1e-3)) for k, v in m.items()},
            "libjpeg_over_model": round(m["mixed_rgb_libjpeg"] / m["mixed_rgb_model"], 4),
            "loop_over_mixed_libjpeg": round(m["loop_of_jpeg_decode_rgb_libjpeg"] / m["mixed_rgb_libjpeg"], 3), "verified": bool(ok)}


def section_resized(args, hvc, torch, uni, mix, files, distinct):
    n, S = len(files), 224
    lay = hvc.hvc.jpeg_mixed_layout(files)
    out = np.zeros(n * 3 * S * S, dtype=np.uint8)

    def mixed(setting):
        mix.set_mixed_arithmetic(setting)
        return mix.jpeg_decode_batch_mixed_resized(files, size=(S, S), filter="bilinear", threads=args.threads, mixed_layout=lay, out=out)
    status, tensor = mixed("libjpeg")
    ok = all(s == 0 for s in status)
    for i in range(0, n, max(1, n // 4)):                       # a sample: Pillow's resize (tools/resize_reference.py) of the per-file image
        ok &= bool(np.array_equal(tensor[i], rr.resize(uni.jpeg_decode_rgb(files[i])[1], S, S, "bilinear")))
    wall = walls({"mixed_resized_model": lambda: mixed("model"), "mixed_resized_libjpeg": lambda: mixed("libjpeg")}, args.runs, mix.synchronize)
    m = {k: float(np.median(v)) for k, v in wall.items()}
    return {"files": n, "distinct": distinct, "size": [S, S], "filter": "bilinear", "wall_ms": {k: round(v, 2) for k, v in m.items()},
            "files_per_s": {k: round(n / (v * 1e-3)) for k, v in m.items()},
            "libjpeg_over_model": round(m["mixed_resized_libjpeg"] / m["mixed_resized_model"], 4), "verified": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="block,colour,files,resized")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    sections = [s for s in args.sections.split(",") if s]
    res = {"kernel_id": hvc.hvc.kernel_build_id(), "runs": args.runs}
    uni, mix = hvc.Context(0), hvc.Context(0)   # the uniform calls under hvc_set_arithmetic(libjpeg); the mixed calls under either mixed setting
    uni.set_arithmetic("libjpeg")
    try:
        if "block" in sections or "colour" in sections:
            for c in (uni, mix):
                c.set_stream(torch.cuda.current_stream().cuda_stream)
            U = Uniform(hvc, torch, mix, args.frames)
            res["block"], d_planes = section_block(args, hvc, torch, uni, mix, U)   # (leaves the libjpeg planes behind: the colour pass's input)
            if "colour" in sections:
                res["colour"] = section_colour(args, hvc, torch, uni, mix, U, d_planes)
            if "block" not in sections:
                del res["block"]
            for c in (uni, mix):
                c.synchronize()
                c.reset_stream()
            del U, d_planes
            torch.cuda.empty_cache()
        if "files" in sections or "resized" in sections:
            distinct, _ = mixed_file_set(mix, min(args.distinct, args.files))
            files = [distinct[i % len(distinct)] for i in range(args.files)]
            if "files" in sections:
                res["files"] = section_files(args, hvc, torch, uni, mix, files, len(distinct))
            if "resized" in sections:
                res["resized"] = section_resized(args, hvc, torch, uni, mix, files, len(distinct))
    finally:
        uni.close()
        mix.close()
    ok = all(v["verified"] for v in res.values() if isinstance(v, dict))
    res["verified"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
