#!/usr/bin/env python3
"""The libjpeg-exact encoder's kernels (hvc_set_encode_libjpeg; csrc/hvc_libjpeg_encode.hip) against the model's kernels in
the same process, on BASELINE's configuration-5 workload: a batch of 4K 4:2:0 pixel records resident in HBM (256 frames by
default, `distinct` seeded frames repeated), quality 75, coefficient records in HBM.  The compared kernels alternate; every
figure is the median of `rounds` rounds of `steps` launches timed with device events.  Prints one JSON line:

  uniform      k_fdct_islow against k_encode: hvc_encode_frames, device events around the kernel
  mixed        k_fdct_islow_mixed against k_encode_mixed: hvc_encode_frames_mixed over the same records as a set of frames whose
               infos state no size (no dummy block), device events around the kernel
  dummy_pass   hvc_encode_frames_mixed, whole calls, over frames of 3832 x 2152 (a dummy column and a dummy row of luma blocks)
               with their sizes stated and with the sizes left out: the difference is k_dummy_blocks_mixed and its host list
  rgb_pass     k_rgb_to_ycc_libjpeg against k_rgb_to_ycc: hvc_rgb_to_yuv on 1024 x 1080p 4:2:0 in device memory, whole calls (one launch)
  verified     the records of the distinct frames equal tools/libjpeg_encode_reference.py's (every coefficient of a sample of
               block rows, both calls), the dummy blocks of frame 0 follow the rule, the planes of the two distinct images equal the definition's

    python tools/bench_libjpeg_encode.py [--frames 256] [--steps 10] [--warmup 3] [--rounds 5] [--distinct 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--rgb-frames", dest="rgb_frames", type=int, default=1024)
    args = ap.parse_args()
    import torch
    import video_coding_amd as hvc
    from video_coding_amd.synth import synth_frame_pixels
    import libjpeg_encode_reference as ler
    planes = [(480, 270, 0), (240, 135, 1), (240, 135, 1)]
    qtabs = np.stack([hvc.hvc.quant_table(0, 75), hvc.hvc.quant_table(1, 75)]).astype(np.uint16)
    specs, cfs, pfs = hvc.hvc.frame_layout(planes)
    comps = hvc.hvc.components(specs)
    ctx = hvc.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    host = np.stack([synth_frame_pixels(50 + 8 * f, planes) for f in range(args.distinct)])
    n = args.frames
    d_pix = torch.from_numpy(host).cuda().repeat((n + args.distinct - 1) // args.distinct, 1)[:n].contiguous()
    d_coefs = torch.zeros((n, cfs), dtype=torch.int16, device="cuda")

    # the same records as a mixed set; sizes: None = the infos state none, else (width, height) of every frame
    def mixed_infos(size):
        infos = (hvc.hvc.JpegInfo * n)()
        for f in range(n):
            info = infos[f]
            info.n_comp, info.n_qtabs = 3, 2
            for t in range(2):
                for k in range(64):
                    info.qtabs[t][k] = int(qtabs[t][k])
            for i, s in enumerate(specs):
                L = info.layout[i]
                L.blocks_w, L.blocks_h, L.qtab = s["blocks_w"], s["blocks_h"], s["qtab"]
                L.coef_offset, L.plane_offset, L.stride = s["coef_offset"], s["plane_offset"], s["stride"]
                info.comp[i].hscale = info.comp[i].vscale = 2 if i == 0 else 1
                if size:
                    info.comp[i].actual_width, info.comp[i].actual_height = (size[0], size[1]) if i == 0 else (size[0] // 2, size[1] // 2)
            info.coef_count, info.pixel_bytes = cfs, pfs
            if size:
                info.width, info.height = size
        return infos

    po, co = [f * pfs for f in range(n)], [f * cfs for f in range(n)]
    plain, sized = mixed_infos(None), mixed_infos((3832, 2152))

    def kernel_ms(libjpeg, mixed):
        ctx.set_encode_libjpeg(libjpeg)
        ctx.set_profiling(True)
        call = (lambda: ctx.encode_frames_mixed(d_pix.view(-1), po, plain, d_coefs.view(-1), co)) if mixed else \
            (lambda: ctx.encode_frames(d_pix, pfs, qtabs, comps, n, d_coefs, cfs))
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize()
        ms = float(np.median(ctx.kernel_ms_history(min(args.steps, 64))))
        ctx.set_profiling(False)
        return ms

    def call_ms(infos):
        ctx.set_encode_libjpeg(True)
        for _ in range(args.warmup):
            ctx.encode_frames_mixed(d_pix.view(-1), po, infos, d_coefs.view(-1), co)
        ctx.synchronize()
        ctx.timer_begin()
        for _ in range(args.steps):
            ctx.encode_frames_mixed(d_pix.view(-1), po, infos, d_coefs.view(-1), co)
        return ctx.timer_end() / args.steps

    out = {k: [] for k in ("k_encode", "k_fdct_islow", "k_encode_mixed", "k_fdct_islow_mixed", "sized", "unsized")}
    for _ in range(max(1, args.rounds)):
        out["k_encode"].append(kernel_ms(False, False))
        out["k_fdct_islow"].append(kernel_ms(True, False))
        out["k_encode_mixed"].append(kernel_ms(False, True))
        out["k_fdct_islow_mixed"].append(kernel_ms(True, True))
        out["unsized"].append(call_ms(plain))
        out["sized"].append(call_ms(sized))
    med = {k: float(np.median(v)) for k, v in out.items()}

    # verified on a sample: block rows 0, 133 and the last but one of every plane of the distinct frames, uniform and mixed call
    def sample_ok(records):
        for f in range(args.distinct):
            for s in specs:
                bw, bh = s["blocks_w"], s["blocks_h"]
                plane = host[f, s["plane_offset"]:s["plane_offset"] + s["stride"] * bh * 8].reshape(bh * 8, s["stride"])
                rec = records[f, s["coef_offset"]:s["coef_offset"] + bw * bh * 64].reshape(bh, bw * 64)
                for by in (0, min(133, bh - 1), bh - 2):   # (not the last row and column: dummies where the sizes are stated)
                    want = ler.fdct_quant_plane(plane[by * 8:by * 8 + 8, :(bw - 1) * 8], qtabs[s["qtab"]]).reshape(-1)
                    if not np.array_equal(rec[by, :(bw - 1) * 64], want):
                        return False
        return True

    ctx.set_encode_libjpeg(True)
    ctx.encode_frames(d_pix, pfs, qtabs, comps, n, d_coefs, cfs)
    ctx.synchronize()
    ok_uniform = sample_ok(d_coefs[:args.distinct].cpu().numpy())
    d_coefs.zero_()
    ctx.encode_frames_mixed(d_pix.view(-1), po, sized, d_coefs.view(-1), co)
    ctx.synchronize()
    got = d_coefs[:args.distinct].cpu().numpy()
    ok_mixed = sample_ok(got)
    luma = got[0, :480 * 270 * 64].reshape(270, 480, 64)
    ok_dummy = (not luma[269, :, 1:].any()) and (not luma[:, 479, 1:].any()) and \
        all(luma[269, bx, 0] == luma[268, min(bx // 2 * 2 + 1, 478), 0] for bx in range(480)) and \
        all(luma[by, 479, 0] == luma[by, 478, 0] for by in range(269))
    # the colour pass: hvc_rgb_to_yuv on 1024 x 1080p 4:2:0, device memory, whole calls (one launch each), the setting on and off
    rw, rh, rn = 1920, 1080, args.rgb_frames
    rng = np.random.default_rng(77)
    img = rng.integers(0, 256, size=(2, rh, rw, 3), dtype=np.uint8)
    d_rgb = torch.from_numpy(img).cuda().repeat((rn + 1) // 2, 1, 1, 1)[:rn].contiguous()
    rspecs, _, rfs = hvc.hvc.frame_layout([(240, 135, 0), (120, 68, 1), (120, 68, 1)])
    d_yuv = torch.zeros((rn, rfs), dtype=torch.uint8, device="cuda")

    def rgb_ms(libjpeg):
        ctx.set_encode_libjpeg(libjpeg)
        for _ in range(args.warmup):
            ctx.rgb_to_yuv(d_rgb, rw, rh, 420, d_yuv, rspecs, n_frames=rn, yuv_frame_stride=rfs)
        ctx.synchronize()
        ctx.timer_begin()
        for _ in range(args.steps):
            ctx.rgb_to_yuv(d_rgb, rw, rh, 420, d_yuv, rspecs, n_frames=rn, yuv_frame_stride=rfs)
        return ctx.timer_end() / args.steps

    rgb_out = {"k_rgb_to_ycc": [], "k_rgb_to_ycc_libjpeg": []}
    for _ in range(max(1, args.rounds)):
        rgb_out["k_rgb_to_ycc"].append(rgb_ms(False))
        rgb_out["k_rgb_to_ycc_libjpeg"].append(rgb_ms(True))   # (last: d_yuv holds its planes)
    got_yuv = d_yuv[:2].cpu().numpy()
    ok_rgb = True
    for f in range(2):
        for sp, p in zip(rspecs, ler.rgb_to_planes(img[f], 420)):
            ah, aw = (rh, rw) if sp is rspecs[0] else (rh // 2, rw // 2)
            plane = got_yuv[f, sp["plane_offset"]:sp["plane_offset"] + sp["stride"] * ah].reshape(ah, sp["stride"])
            ok_rgb = ok_rgb and np.array_equal(plane[:, :aw], p[:ah, :aw])
    rmed = {k: float(np.median(v)) for k, v in rgb_out.items()}
    ctx.close()
    r = lambda x: round(x, 4)
    print(json.dumps({
        "config": "libjpeg-encode-5", "frames": n, "steps": args.steps, "rounds": args.rounds,
        "uniform": {"k_encode_ms": r(med["k_encode"]), "k_fdct_islow_ms": r(med["k_fdct_islow"]),
                    "ratio": r(med["k_fdct_islow"] / med["k_encode"]), "rounds": {k: [r(x) for x in out[k]] for k in ("k_encode", "k_fdct_islow")}},
        "mixed": {"k_encode_mixed_ms": r(med["k_encode_mixed"]), "k_fdct_islow_mixed_ms": r(med["k_fdct_islow_mixed"]),
                  "ratio": r(med["k_fdct_islow_mixed"] / med["k_encode_mixed"]),
                  "rounds": {k: [r(x) for x in out[k]] for k in ("k_encode_mixed", "k_fdct_islow_mixed")}},
        "dummy_pass": {"call_ms_sizes_stated": r(med["sized"]), "call_ms_no_sizes": r(med["unsized"]),
                       "share": r((med["sized"] - med["unsized"]) / med["sized"]), "dummies_per_frame": 480 + 269},
        "rgb_pass": {"frames": rn, "k_rgb_to_ycc_ms": r(rmed["k_rgb_to_ycc"]), "k_rgb_to_ycc_libjpeg_ms": r(rmed["k_rgb_to_ycc_libjpeg"]),
                     "ratio": r(rmed["k_rgb_to_ycc_libjpeg"] / rmed["k_rgb_to_ycc"]), "rounds": {k: [r(x) for x in v] for k, v in rgb_out.items()}},
        "verified": {"uniform_sample": bool(ok_uniform), "mixed_sample": bool(ok_mixed and ok_dummy), "rgb_planes": bool(ok_rgb)}}))


if __name__ == "__main__":
    main()
