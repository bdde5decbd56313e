"""Measures the resizing step (include/hvc_jpeg.h, Resizing) -- one process, calls alternating, medians of 5, every output
verified against tools/resize_reference.py on a sample.  Prints one JSON line.

  passes   (a) hvc_rgb_resize_mixed alone on --images RGB images of 1920 x 1080 -> 224 x 224 in device memory, each filter:
           device events around the call; against the byte model (source read + intermediate written and read + destination
           written) and against one torch.nn.functional.interpolate(..., antialias=True) per image -- what a caller does
           today; a different arithmetic, compared for time only
  files    (b) the seeded file set of tools/bench_mixed.py through hvc_jpeg_decode_batch_mixed_resized to a 224 x 224 tensor in
           host memory, at scale_denom 1 and at the largest denominator that keeps every image at least 224 wide and high;
           against hvc_jpeg_decode_batch_mixed_rgb of the same run, and against that call followed by a host loop of
           Pillow's Image.resize ("not measured" where Pillow does not import)
           (c) the resize's share of one chunk's kernel time: the two passes (profiling pair) over the images of the first
           chunk against the batch call's kernel_ms_sum per chunk

    python tools/bench_resize.py [--sections passes,files] [--images 1024] [--files 4096] [--distinct 256] [--threads 16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import resize_reference as rr  # noqa: E402
from bench_mixed import mixed_file_set  # noqa: E402

FILTERS = ("box", "bilinear", "bicubic")
REPS = 5


def section_passes(args, hvc, torch, ctx):
    n, (w, h), (W, H) = args.images, (1920, 1080), (224, 224)
    distinct = 8   # (distinct contents: the timing does not depend on them, the verification does)
    rng = np.random.Generator(np.random.PCG64(20261020))
    base = rng.integers(0, 256, size=(distinct, h, w, 3), dtype=np.uint8)
    src = torch.from_numpy(base).cuda().repeat((n + distinct - 1) // distinct, 1, 1, 1)[:n].contiguous()
    dst = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    s_off, d_off = [i * 3 * w * h for i in range(n)], [i * 3 * W * H for i in range(n)]
    out = {"images": n, "from": [w, h], "to": [W, H], "filters": {}}
    ok = True
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    chw = src[:distinct].permute(0, 3, 1, 2).float().contiguous()   # what the torch caller would hold

    def ours(filt):
        ctx.rgb_resize_mixed(src.view(-1), s_off, [w] * n, [h] * n, dst.view(-1), d_off, [W] * n, [H] * n, filter=filt)

    def theirs(filt):
        mode = {"box": "area", "bilinear": "bilinear", "bicubic": "bicubic"}[filt]
        kw = {} if mode == "area" else {"antialias": True, "align_corners": False}
        for i in range(n):
            torch.nn.functional.interpolate(chw[i % distinct:i % distinct + 1], size=(H, W), mode=mode, **kw)

    for filt in FILTERS:
        ours(filt)
        torch.cuda.synchronize()
        got = dst[:distinct].cpu().numpy()
        ok &= all(np.array_equal(got[i], rr.resize(base[i], W, H, filt)) for i in (0, distinct - 1))
        ok &= bool(np.array_equal(dst[n - 1].cpu().numpy(), rr.resize(base[(n - 1) % distinct], W, H, filt)))
        ms = {"hvc_rgb_resize_mixed": [], "interpolate_per_image": []}
        for _ in range(REPS):
            for name, fn in (("hvc_rgb_resize_mixed", ours), ("interpolate_per_image", theirs)):
                e0.record()
                fn(filt)
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        ctx.set_profiling(True)   # the two launches alone (the events above also see the host's plan in front of them)
        k_ms = []
        for _ in range(REPS):
            ours(filt)
            ctx.synchronize()
            k_ms.append(ctx.last_kernel_ms())
        ctx.set_profiling(False)
        med["both_passes_kernel_time"] = float(np.median(k_ms))
        model = n * (3 * w * h + 2 * 3 * W * h + 3 * W * H)   # source + intermediate written and read + destination
        out["filters"][filt] = {"ms": {k: round(v, 3) for k, v in med.items()}, "model_MB": round(model / 1e6, 1),
                                "model_TBps": round(model / (med["both_passes_kernel_time"] * 1e-3) / 1e12, 3),
                                "interpolate_over_ours": round(med["interpolate_per_image"] / med["hvc_rgb_resize_mixed"], 3)}
    out["verified"] = bool(ok)
    return out


def section_files(args, hvc, torch, ctx):
    n, (W, H) = args.files, (224, 224)
    distinct, keys = mixed_file_set(ctx, min(args.distinct, n))
    files = [distinct[i % len(distinct)] for i in range(n)]
    small = min(min(k[0], k[1]) for k in keys)
    denom = max(d for d in (1, 2, 4, 8) if -(-small // d) >= 224 or d == 1)
    lay = hvc.hvc.jpeg_mixed_layout(files)
    rlay = hvc.hvc.jpeg_mixed_rgb_layout(files)
    rbuf = np.zeros(rlay.total_bytes, dtype=np.uint8)
    tensor = np.zeros(n * 3 * W * H, dtype=np.uint8)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    out = {"files": n, "distinct": len(distinct), "threads": args.threads, "to": [W, H], "smallest_side": small, "largest_denom": denom,
           "full_size_rgb_MB": round(rlay.total_bytes / 1e6, 1), "tensor_MB": round(tensor.size / 1e6, 1), "scales": {}}
    ok = True

    def rgb_call():
        return ctx.jpeg_decode_batch_mixed_rgb(files, threads=args.threads, rgb_layout=rlay, rgb=rbuf)

    def rgb_then_pillow():
        res = rgb_call()
        return [np.asarray(Image.fromarray(np.ascontiguousarray(r[2])).resize((W, H), Image.BILINEAR)) for r in res]

    for scale in sorted({1, denom}):
        def resized():
            return ctx.jpeg_decode_batch_mixed_resized(files, size=(W, H), filter="bilinear", scale_denom=scale, threads=args.threads,
                                                       mixed_layout=lay, out=tensor)
        status, t = resized()
        st = ctx.last_batch_stats
        ok &= all(s == 0 for s in status)
        for i in (0, len(distinct) // 2, len(distinct) - 1, n - 1):
            one = ctx.jpeg_decode_rgb(files[i])[1] if scale == 1 else ctx.jpeg_decode_scaled_rgb(files[i], scale)[1]
            ok &= bool(np.array_equal(t[i], rr.resize(one, W, H, "bilinear")))
        calls = {"batch_mixed_resized": resized, "batch_mixed_rgb": rgb_call}
        if Image is not None and scale == 1:
            calls["batch_mixed_rgb_then_pillow_resize"] = rgb_then_pillow
        wall = {k: [] for k in calls}
        for _ in range(REPS):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                ctx.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(v)) for k, v in wall.items()}
        if "batch_mixed_rgb_then_pillow_resize" not in med:
            med["batch_mixed_rgb_then_pillow_resize"] = None
        # (c) the passes over the first chunk's images, alone, by the profiling pair
        first = max(1, n // max(1, st.chunks))
        infos = [lay.infos[i] for i in range(first)]
        dims = [(-(-i.width // scale), -(-i.height // scale)) for i in infos]
        s_off, at = [], 0
        for w, h in dims:
            s_off.append(at)
            at += 3 * w * h
        d_src = torch.zeros(at, dtype=torch.uint8, device="cuda")
        d_dst = torch.zeros(first * 3 * W * H, dtype=torch.uint8, device="cuda")
        ctx.set_profiling(True)
        k_ms = []
        for _ in range(REPS):
            ctx.rgb_resize_mixed(d_src, s_off, [d[0] for d in dims], [d[1] for d in dims], d_dst, [i * 3 * W * H for i in range(first)],
                                 [W] * first, [H] * first, filter="bilinear")
            ctx.synchronize()
            k_ms.append(ctx.last_kernel_ms())
        ctx.set_profiling(False)
        per_chunk = st.kernel_ms_sum / max(1, st.chunks)
        out["scales"][str(scale)] = {
            "chunks": st.chunks, "entropy_ms_sum": round(st.entropy_ms_sum, 1), "kernel_ms_sum": round(st.kernel_ms_sum, 2),
            "wall_ms": {k: (round(v, 2) if v is not None else "not measured") for k, v in med.items()},
            "files_per_s": {k: (round(n / (v * 1e-3)) if v is not None else "not measured") for k, v in med.items()},
            "rgb_over_resized": round(med["batch_mixed_rgb"] / med["batch_mixed_resized"], 3),
            "resize_ms_first_chunk": round(float(np.median(k_ms)), 3), "kernel_ms_per_chunk": round(per_chunk, 3),
            "resize_share_of_chunk_kernel_time": round(float(np.median(k_ms)) / per_chunk, 3) if per_chunk > 0 else "not measured"}
    out["verified"] = bool(ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="passes,files")
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    sections = {"passes": section_passes, "files": section_files}
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
