"""A closed context gives its device memory back.

One cycle creates a context, runs a sized call and then one smallest-shape call of every family (so that every buffer,
event and stream the context can own is created in each of its forms), and closes it.  After a warm-up cycle (the
runtime's one-time allocations) four more cycles must not lower the free device memory by S / 2 or more, S being what the
sized call makes the context hold.

Why S / 2: the sized call is a host-memory decode_frames of one single-component frame of 256 x 256 blocks, 8 MiB of
coefficient records and 4 MiB of pixels, which the context stages in its two block-stage buffers, grown with a quarter
plus 4096 bytes to spare: S = 12 MiB * 5 / 4 + 8192 bytes, about 15 MiB.  Losing those two buffers once costs S, losing
them every cycle 4 S; S / 2 lies below either and far above what the runtime's own bookkeeping drifts by between cycles.
Measured on an MI355X when the test was written: 0 bytes of drift in each of the four cycles, with hvc_destroy releasing every
field by hand and with the owning types alike; a build whose buffers are never released lost 23 068 672 bytes in the first
cycle and failed here.

What this does not cover: a leaked buffer smaller than the allocator's granularity does not move the free-memory figure
and is not caught.  The test guards against the gross mistake; the owning types of csrc/hvc_ctx.h, whose destructors
release what a context member holds, are what exclude the small ones.

Every call takes host (numpy) memory, so torch's caching allocator holds nothing that could mask or mimic a leak."""
import numpy as np
import pytest

from batch_files import mixed_files, uniform_files
from oracle import orc

pytestmark = pytest.mark.gpu

SIDE = 256                                        # blocks per side of the sized frame
COEF_BYTES, PIXEL_BYTES = SIDE * SIDE * 128, SIDE * SIDE * 64
S = (COEF_BYTES + PIXEL_BYTES) * 5 // 4 + 2 * 4096


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _cycle(hvc, d):
    c = hvc.Context(0)
    try:
        spec = [dict(blocks_w=SIDE, blocks_h=SIDE, qtab=0, coef_offset=0, plane_offset=0, stride=SIDE * 8)]
        c.decode_frames(d["big"], d["big"].size, d["q"], spec, 1, np.zeros(PIXEL_BYTES, np.uint8), PIXEL_BYTES)
        jpegs, fs = d["jpegs"], d["fs"]
        c.jpeg_decode(jpegs[0])
        for gpu in (False, True):
            c.jpeg_decode_batch(jpegs, np.zeros(len(jpegs) * fs, np.uint8), fs, threads=2, frames_per_chunk=2, gpu_entropy=gpu)
        c.jpeg_decode_batch_mixed(d["mixed"], threads=2)
        c.jpeg_decode_batch_mixed_rgb(d["mixed"], threads=2)
        c.set_mixed_reader("gpu")
        c.jpeg_decode_batch_mixed(d["mixed"], threads=2)
        c.jpeg_decode_batch_mixed_rgb(d["mixed"], threads=2)
        for gpu in (False, True):
            c.jpeg_encode_batch(d["raw"], 64, 64, 420, 75, threads=2, frames_per_chunk=2, gpu_entropy=gpu)
        c.huffman_encode_frames_optimised(d["info"], d["rec"], d["info"].coef_count, 1, restart_interval=3)
        c.dct_fixed("forward", 12, 2, d["blocks"])
        small = [dict(blocks_w=3, blocks_h=2, qtab=0, coef_offset=0, plane_offset=0, stride=24)]
        c.decode_divergence(d["big"][:2 * 384], 384, d["q"], small, 2)
        px = np.zeros(2 * 384, np.uint8)
        c.decode_frames_submit(0, d["big"][:2 * 384], 384, d["q"], small, 2, px, 384)
        c.wait(0)
    finally:
        c.close()


def test_a_closed_context_gives_its_device_memory_back():
    import video_coding_amd as hvc
    rng = np.random.default_rng(11)
    jpegs, frames = uniform_files(4, 31000)
    info = hvc.hvc.jpeg_encoder_layout(64, 64, 420, 75)
    _, coefs = orc.encode_yuv(*frames[0], 64, 64, 420, 75, want_coefs=True)
    d = dict(big=rng.integers(-60, 61, COEF_BYTES // 2).astype(np.int16), q=rng.integers(1, 256, (1, 64)).astype(np.uint16),
             jpegs=jpegs, fs=hvc.hvc.jpeg_read_header(jpegs[0]).pixel_bytes, mixed=mixed_files(),
             raw=[np.concatenate([p.reshape(-1) for p in f]) for f in frames], info=info,
             rec=np.concatenate([c.reshape(-1) for c in coefs]).astype(np.int16),
             blocks=rng.integers(-255, 256, (4, 8, 8)).astype(np.int32))
    _cycle(hvc, d)
    base = _free_bytes()
    for i in range(4):
        _cycle(hvc, d)
        free = _free_bytes()
        print("cycle %d: free memory %+d bytes against the warm-up's (S = %d)" % (i + 1, free - base, S))
        assert base - free < S // 2, (i, base - free, S)
