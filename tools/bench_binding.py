"""Wall time per call of the binding methods that share a tail (mixed batch decode and encode, the GPU Huffman coder wrappers),
on a small file set where the time in Python shows: python tools/bench_binding.py [TREE] (default: this tree; another checkout
to compare two bindings over one library).  Median ms of CALLS calls per line, one JSON line.  Never part of bench.py's value."""
import json
import os
import sys
import time

tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, tree)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import video_coding_amd as hvc  # noqa: E402

H = hvc.hvc
GOLDEN = os.path.join(tree, "tests", "golden")
CALLS = 15


def rd(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def timed(fn):
    fn()
    fn()
    ms = []
    for _ in range(CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 4)


def main():
    assert os.path.dirname(os.path.abspath(H.__file__)).startswith(tree), H.__file__
    ctx = hvc.Context(0)
    mini, mouse = rd("mini.jpg"), rd("Mouse480.jpg")
    files = [mini, mouse] * 32
    out = {"tree": tree, "kernels": H.kernel_build_id()}
    lay = H.MixedLayout(files)
    host = np.zeros(lay.total_bytes, dtype=np.uint8)
    dev = torch.zeros(lay.total_bytes, dtype=torch.uint8, device="cuda")
    out["decode_mixed.host.own_buffer"] = timed(lambda: ctx.jpeg_decode_batch_mixed(files, threads=8, layout=lay, pixels=host))
    out["decode_mixed.device.own_buffer"] = timed(lambda: ctx.jpeg_decode_batch_mixed(files, threads=8, layout=lay, pixels=dev))
    out["decode_mixed.host.made_here"] = timed(lambda: ctx.jpeg_decode_batch_mixed(files, threads=8))
    out["decode_mixed_rgb.host.made_here"] = timed(lambda: ctx.jpeg_decode_batch_mixed_rgb(files, threads=8))
    out["decode_mixed_scaled.host.made_here"] = timed(lambda: ctx.jpeg_decode_batch_mixed_scaled(files, 2, threads=8))
    out["decode_mixed_scaled_rgb.device.made_here"] = timed(lambda: ctx.jpeg_decode_batch_mixed_scaled_rgb(files, 2, threads=8, device=True))
    out["decode_mixed_resized.device"] = timed(lambda: ctx.jpeg_decode_batch_mixed_resized(files, size=(64, 64), device=True, threads=8))

    rng = np.random.default_rng(7)
    specs = [(64, 64, 420, 75), (48, 32, 444, 50)] * 16
    raws = [rng.integers(0, 256, w * h * (3 if c == 444 else 3) // (1 if c == 444 else 2), dtype=np.uint8).tobytes() for w, h, c, _ in specs]
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h, _, _ in specs]
    out["encode_mixed.host_coder"] = timed(lambda: ctx.jpeg_encode_batch_mixed(raws, specs, threads=8))
    out["encode_mixed.gpu_coder"] = timed(lambda: ctx.jpeg_encode_batch_mixed_gpu(raws, specs, threads=8))
    out["encode_mixed_rgb.host_coder"] = timed(lambda: ctx.jpeg_encode_batch_mixed_rgb(images, specs, threads=8))
    out["encode_mixed_rgb.gpu_coder"] = timed(lambda: ctx.jpeg_encode_batch_mixed_rgb(images, specs, threads=8, coder="gpu"))

    info, rec = H.jpeg_entropy_decode(mouse)
    n = 8
    recs = np.ascontiguousarray(np.stack([rec] * n))
    d_recs = torch.from_numpy(recs).cuda()
    cc = info.coef_count
    out["huffman.host"] = timed(lambda: ctx.huffman_encode_frames(info, recs, cc, n))
    out["huffman.device"] = timed(lambda: ctx.huffman_encode_frames(info, d_recs, cc, n))
    out["huffman_optimised.device"] = timed(lambda: ctx.huffman_encode_frames_optimised(info, d_recs, cc, n))
    out["huffman_restart.device"] = timed(lambda: ctx.huffman_encode_frames(info, d_recs, cc, n, restart_interval=8))
    offs = [f * cc for f in range(n)]
    flat = d_recs.reshape(-1)
    out["huffman_mixed.device"] = timed(lambda: ctx.huffman_encode_frames_mixed([info] * n, flat, offs))
    out["huffman_mixed_optimised.device"] = timed(lambda: ctx.huffman_encode_frames_mixed([info] * n, flat, offs, optimised=True))
    ctx.close()
    print(json.dumps(out), flush=True)


main()
