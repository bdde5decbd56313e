#!/usr/bin/env python3
"""The mixed batch with the GPU Huffman reader (hvc_set_mixed_reader, csrc/hvc_hdec_mixed.hip) against the same call with the
host reader, in one process, the two settings alternating, every output verified first.  The files are the seeded set of
tools/bench_mixed.py (`--files` files, `--distinct` different ones repeated), host output, `--threads` host threads:

  planes       hvc_jpeg_decode_batch_mixed
  rgb_eighth   hvc_jpeg_decode_batch_mixed_scaled_rgb at 1/8 (the thumbnail form: the reader is nearly all of its work)

Per form and setting: wall times of `--runs` runs (median, minimum, all of them) and the GPU / host split of the files
(hvc_last_mixed_reader_files).  The host setting is the code path of the library without the GPU reader.  Prints one JSON line.
    python tools/bench_mixed_reader.py [--files 4096] [--distinct 256] [--runs 5] [--threads 16]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    from bench_mixed import mixed_file_set
    ctx = hvc.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    res = {"kernel_id": hvc.hvc.kernel_build_id(), "files": args.files, "threads": args.threads, "runs": max(5, args.runs)}
    ok = True
    try:
        distinct, _ = mixed_file_set(ctx, min(args.distinct, args.files))
        files = [distinct[i % len(distinct)] for i in range(args.files)]
        res["distinct"] = len(distinct)
        lay_p = hvc.hvc.MixedLayout(files)
        lay_r = hvc.hvc.MixedScaledRgbLayout(files, 8, "interleaved", 0, 0)
        def span(lay, f):   # where file f's record lies in its form's buffer
            if lay is lay_p:
                return lay.pixel_offsets[f], lay.infos[f].pixel_bytes
            return lay.rgb_offsets[f], (lay.scaled[f].height - 1) * lay.rgb_row_strides[f] + 3 * lay.scaled[f].width

        forms = {
            "planes": (lay_p, lambda buf: ctx.jpeg_decode_batch_mixed(files, threads=args.threads, layout=lay_p, pixels=buf)),
            "rgb_eighth": (lay_r, lambda buf: ctx.jpeg_decode_batch_mixed_scaled_rgb(files, 8, threads=args.threads, rgb_layout=lay_r, rgb=buf)),
        }
        for name, (lay, call) in forms.items():
            bufs = {r: np.zeros(max(lay.total_bytes, 8), dtype=np.uint8) for r in ("host", "gpu")}
            split, status = {}, {}
            for reader in ("host", "gpu"):          # verification (and warm-up: rings, pool, pinned memory)
                ctx.set_mixed_reader(reader)
                status[reader] = [r[0] for r in call(bufs[reader])]
                split[reader] = ctx.last_mixed_reader_files()
            # every file's record (the alignment padding between records is nobody's: a host-output call may overwrite it)
            same = status["host"] == status["gpu"] and all(s == 0 for s in status["host"])
            for f in range(len(files)):
                off, nb = span(lay, f)
                same = same and bool(np.array_equal(bufs["host"][off:off + nb], bufs["gpu"][off:off + nb]))
            ok &= same
            wall = {"host": [], "gpu": []}
            for _ in range(max(5, args.runs)):
                for reader in ("host", "gpu"):
                    ctx.set_mixed_reader(reader)
                    t0 = time.perf_counter()
                    call(bufs[reader])
                    ctx.synchronize()
                    wall[reader].append((time.perf_counter() - t0) * 1e3)
            med = {k: float(np.median(v)) for k, v in wall.items()}
            spread = {k: float(np.max(v) - np.min(v)) for k, v in wall.items()}
            res[name] = {"output_MB": round(lay.total_bytes / 1e6, 1), "chunks": ctx.last_batch_stats.chunks,
                         "wall_ms_median": {k: round(v, 2) for k, v in med.items()},
                         "wall_ms_min": {k: round(float(np.min(v)), 2) for k, v in wall.items()},
                         "wall_ms_runs": {k: [round(x, 1) for x in v] for k, v in wall.items()},
                         "gpu_files_host_files": {k: list(v) for k, v in split.items()},
                         "host_over_gpu": round(med["host"] / med["gpu"], 3),
                         # a gain only where the medians differ by more than the runs of either setting spread
                         "gpu_faster_beyond_spread": bool(med["host"] - med["gpu"] > max(spread.values())),
                         "verified": bool(same)}
    finally:
        ctx.set_mixed_reader("host")
        ctx.close()
    res["verified"] = bool(ok)
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
