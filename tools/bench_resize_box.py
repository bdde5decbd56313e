"""Measures what the option block of the resizing calls costs and saves (include/hvc_jpeg.h, Resizing: Box, Mirror, Typed output)
-- one process, calls alternating, medians of 5, every output verified against tools/resize_reference.py on a sample.  Nothing
is gated.  Prints one JSON line.

  typed    (a) the vertical pass alone on --images images of 224 x 1080 -> 224 x 224 in device memory (what the vertical pass
           of tools/bench_resize.py's 1920 x 1080 -> 224 x 224 works on: the horizontal axis is skipped, so the profiling pair
           brackets k_resize_v_mixed, or k_resize_v_mixed_lut<2> / <4> under a typed output, and nothing else), both layouts
  files    (b) the seeded file set of tools/bench_mixed.py with a seeded RandomResizedCrop box and a coin-flip mirror per file
           through hvc_jpeg_decode_batch_mixed_resized_opts to a planar float16 [n, 3, 224, 224] device tensor, against the call
           without options (whole images, uint8 [n, 224, 224, 3]) followed by torch's permute / float / normalise / half --
           another picture (no crop), compared for time only
           (c) the source rows the row window saves the horizontal pass over those boxes (counted from the definition), and
           the two passes alone (profiling pair) over the first chunk's images with and without the boxes

    python tools/bench_resize_box.py [--sections typed,files] [--images 1024] [--files 4096] [--distinct 256] [--threads 16]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import resize_reference as rr  # noqa: E402
from bench_mixed import mixed_file_set  # noqa: E402

REPS = 5
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def section_typed(args, hvc, torch, ctx):
    n, (w, h), (W, H) = args.images, (224, 1080), (224, 224)
    distinct = 8
    rng = np.random.Generator(np.random.PCG64(20261021))
    base = rng.integers(0, 256, size=(distinct, h, w, 3), dtype=np.uint8)
    out = {"images": n, "from": [w, h], "to": [W, H], "filter": "bilinear", "layouts": {}}
    ok = True
    luts = {2: hvc.normalize_lut(*IMAGENET, "float16"), 4: hvc.normalize_lut(*IMAGENET, "float32")}
    for layout in ("interleaved", "planar"):
        imgs = base if layout == "interleaved" else np.ascontiguousarray(base.transpose(0, 3, 1, 2))
        src = torch.from_numpy(imgs).cuda().repeat((n + distinct - 1) // distinct, 1, 1, 1)[:n].contiguous().view(-1)
        s_off = [i * 3 * w * h for i in range(n)]
        res = {}
        for elem in (1, 2, 4):
            dst = torch.zeros(n * 3 * W * H * elem, dtype=torch.uint8, device="cuda")
            d_off = [i * 3 * W * H * elem for i in range(n)]
            kw = {"lut": luts[elem]} if elem > 1 else {}

            def call():
                ctx.rgb_resize_mixed(src, s_off, [w] * n, [h] * n, dst, d_off, [W] * n, [H] * n, filter="bilinear", layout=layout, **kw)

            call()
            ctx.synchronize()
            for i in (0, n - 1):
                want = rr.resize_box(base[i % distinct], W, H, "bilinear")
                want = rr.apply_lut(want, luts[elem]) if elem > 1 else want
                want = np.ascontiguousarray(want.transpose(2, 0, 1)) if layout == "planar" else want
                got = dst[d_off[i]:d_off[i] + 3 * W * H * elem].cpu().numpy()
                ok &= bool(np.array_equal(got, want.reshape(-1).view(np.uint8)))
            ctx.set_profiling(True)
            ms = []
            for _ in range(REPS):
                call()
                ctx.synchronize()
                ms.append(ctx.last_kernel_ms())
            ctx.set_profiling(False)
            med = float(np.median(ms))
            model = n * (3 * w * h + 3 * W * H * elem)            # source read + destination written
            res[{1: "k_resize_v_mixed", 2: "k_resize_v_mixed_lut<2>", 4: "k_resize_v_mixed_lut<4>"}[elem]] = {
                "ms": round(med, 3), "model_MB": round(model / 1e6, 1), "model_TBps": round(model / (med * 1e-3) / 1e12, 3)}
            del dst
        base_ms = res["k_resize_v_mixed"]["ms"]
        for k in ("k_resize_v_mixed_lut<2>", "k_resize_v_mixed_lut<4>"):
            res[k]["over_uint8"] = round(res[k]["ms"] / base_ms, 3)
        out["layouts"][layout] = res
        del src
        torch.cuda.empty_cache()
    out["verified"] = bool(ok)
    return out


def random_resized_crop(rng, w, h, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision's RandomResizedCrop.get_params on a seeded generator: (x0, y0, x1, y1), integers"""
    area = w * h
    for _ in range(10):
        target = area * rng.uniform(*scale)
        aspect = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        cw, ch = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            x0, y0 = int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1))
            return (float(x0), float(y0), float(x0 + cw), float(y0 + ch))
    cw, ch = min(w, h), min(w, h)                               # (the fallback, simplified: the central square)
    return (float((w - cw) // 2), float((h - ch) // 2), float((w - cw) // 2 + cw), float((h - ch) // 2 + ch))


def section_files(args, hvc, torch, ctx):
    n, (W, H) = args.files, (224, 224)
    distinct, keys = mixed_file_set(ctx, min(args.distinct, n))
    files = [distinct[i % len(distinct)] for i in range(n)]
    lay = hvc.hvc.jpeg_mixed_layout(files)
    rng = np.random.Generator(np.random.PCG64(20261021))
    boxes = [random_resized_crop(rng, lay.infos[f].width, lay.infos[f].height) for f in range(n)]
    mirror = [bool(v) for v in rng.integers(0, 2, size=n)]
    typed = torch.zeros(n * 3 * W * H * 2, dtype=torch.uint8, device="cuda")
    plain = torch.zeros(n * 3 * W * H, dtype=torch.uint8, device="cuda")
    mean = torch.tensor(IMAGENET[0], device="cuda")[None, :, None, None]
    std = torch.tensor(IMAGENET[1], device="cuda")[None, :, None, None]
    ok = True

    def fused():
        return ctx.jpeg_decode_batch_mixed_resized(files, size=(W, H), filter="bilinear", layout="planar", device=True, threads=args.threads,
                                                   mixed_layout=lay, out=typed, boxes=boxes, mirror=mirror, dtype="float16",
                                                   mean=IMAGENET[0], std=IMAGENET[1])

    def existing_then_torch():
        status, t = ctx.jpeg_decode_batch_mixed_resized(files, size=(W, H), filter="bilinear", device=True, threads=args.threads, mixed_layout=lay,
                                                        out=plain)
        ctx.synchronize()
        return status, ((t.permute(0, 3, 1, 2).float() / 255 - mean) / std).half()

    status, t = fused()
    ctx.synchronize()
    st = ctx.last_batch_stats
    ok &= all(s == 0 for s in status) and t.dtype == torch.float16 and tuple(t.shape) == (n, 3, H, W)
    lut = hvc.normalize_lut(*IMAGENET, "float16")
    for i in (0, len(distinct) // 2, len(distinct) - 1, n - 1):
        want = rr.apply_lut(rr.resize_box(ctx.jpeg_decode_rgb(files[i])[1], W, H, "bilinear", boxes[i], mirror[i]), lut).transpose(2, 0, 1)
        ok &= bool(np.array_equal(t[i].cpu().numpy().view(np.uint16), np.ascontiguousarray(want).view(np.uint16)))
    calls = {"resized_opts_to_planar_f16": fused, "resized_then_torch_permute_float_normalise_half": existing_then_torch}
    wall = {k: [] for k in calls}
    for _ in range(REPS):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    # (c) the rows of the horizontal pass: every source row without a window, the vertical pass's window with one
    rows_all = sum(lay.infos[f].height for f in range(n))
    rows_win = 0
    for f in range(n):
        lo, hi = rr.row_window(lay.infos[f].height, H, "bilinear", boxes[f][1], boxes[f][3])
        rows_win += hi - lo
    first = max(1, n // max(1, st.chunks))
    dims = [(lay.infos[i].width, lay.infos[i].height) for i in range(first)]
    s_off, at = [], 0
    for w, h in dims:
        s_off.append(at)
        at += 3 * w * h
    d_src = torch.zeros(at, dtype=torch.uint8, device="cuda")
    d_dst = torch.zeros(first * 3 * W * H, dtype=torch.uint8, device="cuda")
    passes = {}
    for name, kw in (("whole_images", {}), ("boxes", {"boxes": boxes[:first]})):
        ctx.set_profiling(True)
        k_ms = []
        for _ in range(REPS):
            ctx.rgb_resize_mixed(d_src, s_off, [d[0] for d in dims], [d[1] for d in dims], d_dst, [i * 3 * W * H for i in range(first)],
                                 [W] * first, [H] * first, filter="bilinear", **kw)
            ctx.synchronize()
            k_ms.append(ctx.last_kernel_ms())
        ctx.set_profiling(False)
        passes[name] = round(float(np.median(k_ms)), 3)
    return {"files": n, "distinct": len(distinct), "threads": args.threads, "to": [W, H], "chunks": st.chunks,
            "tensor_MB": {"planar_f16": round(typed.numel() / 1e6, 1), "uint8": round(plain.numel() / 1e6, 1)},
            "wall_ms": {k: round(v, 2) for k, v in med.items()}, "files_per_s": {k: round(n / (v * 1e-3)) for k, v in med.items()},
            "torch_tail_over_fused": round(med["resized_then_torch_permute_float_normalise_half"] / med["resized_opts_to_planar_f16"], 3),
            "horizontal_rows": {"whole_images": rows_all, "row_window": rows_win, "saved_fraction": round(1 - rows_win / rows_all, 3)},
            "both_passes_first_chunk_ms": dict(passes, images=first), "verified": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="typed,files")
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    sections = {"typed": section_typed, "files": section_files}
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
