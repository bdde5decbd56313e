"""hvc_jpeg_decode_batch_gpu chunk by chunk: seven chunks over a ring of three slots, with chunks the GPU reader must hand to
the host reader at every place of the pipeline -- none, the first, one in the middle, two in a row, the last, all of them --
found out either way the pipeline finds them out:
  at the verdict          a segment cut short (EOI kept): uploaded and read on the GPU, whose 'stream ends early' flag sends the
                          chunk to the host reader, which reads zeros past the end as the model does
  by the worker           restart markers honoured, the batch's first file in intervals, the bad file without any: nothing of
                          the chunk is uploaded, its slot goes straight to the chunk three further on
The pixels must be the host-reader pipeline's byte for byte, into host and into device memory, for a full and a ragged last
chunk; the host reader's time in the stats tells whether a chunk went there."""
import numpy as np
import pytest

from test_gpu_hdec import make_jpeg

pytestmark = pytest.mark.gpu

W = H = 64
CHUNK, THREADS, CHUNKS = 2, 3, 7
BAD_CHUNKS = {"none": (), "first": (0,), "middle": (3,), "two-in-a-row": (2, 3), "last": (6,), "all": tuple(range(CHUNKS))}


@pytest.fixture(scope="module")
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files():
    """14 files of 64 x 64 4:2:0, each in three forms: plain, its segment cut short, and in restart intervals of 4 MCUs"""
    import video_coding_amd as hvc
    plain, cut, marked = [], [], []
    for f in range(CHUNK * CHUNKS):
        j = make_jpeg(900 + 5 * f, W, H, 420, 75)
        info, rec = hvc.hvc.jpeg_entropy_decode(j)
        seg = len(j) - 2 - info.ecs_offset
        c = j[:info.ecs_offset + seg // 2] + b"\xff\xd9"
        hvc.hvc.jpeg_entropy_decode(c)            # the host reader returns records for it (it would raise otherwise)
        m = hvc.hvc.jpeg_entropy_encode(info, rec, restart_interval=4)
        assert np.array_equal(hvc.hvc.jpeg_entropy_decode(m, restart_markers=True)[1], rec)
        plain.append(j)
        cut.append(c)
        marked.append(m)
    return dict(plain=plain, cut=cut, marked=marked)


def batch(files, kind, bad, n):
    """the n files of a case and whether restart markers are honoured for it; the bad file of chunk k is its second one (file 1
    for chunk 0: never file 0, whose probe would send the whole call to the host pipeline), or its only one"""
    good, odd = (files["plain"], files["cut"]) if kind == "verdict" else (files["marked"], files["plain"])
    jpegs = list(good[:n])
    for k in BAD_CHUNKS[bad]:
        f = min(CHUNK * k + 1, n - 1)
        assert f > 0 and f // CHUNK == k
        jpegs[f] = odd[f]
    return jpegs, kind == "worker"


_want = {}


def host_pipeline_pixels(ctx, files, kind, bad, n, fs):
    """what the pipeline with the host reader makes of the case: computed once, shared by the host and device forms"""
    key = (kind, bad, n)
    if key not in _want:
        jpegs, restart = batch(files, kind, bad, n)
        out = np.zeros(n * fs, np.uint8)
        ctx.set_restart_markers(restart)
        try:
            ctx.jpeg_decode_batch(jpegs, out, fs, threads=THREADS, frames_per_chunk=CHUNK, gpu_entropy=False)
        finally:
            ctx.set_restart_markers(False)
        out.setflags(write=False)
        _want[key] = out
    return _want[key]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", [14, 13])
@pytest.mark.parametrize("bad", list(BAD_CHUNKS))
@pytest.mark.parametrize("kind", ["verdict", "worker"])
def test_chunks_handed_to_the_host_reader_anywhere_in_the_pipeline(ctx, files, kind, bad, n, device):
    import torch
    import video_coding_amd as hvc
    fs = hvc.hvc.jpeg_read_header(files["plain"][0]).pixel_bytes
    want = host_pipeline_pixels(ctx, files, kind, bad, n, fs)
    jpegs, restart = batch(files, kind, bad, n)
    out = torch.zeros(n * fs, dtype=torch.uint8, device="cuda") if device else np.zeros(n * fs, np.uint8)
    if device:
        torch.cuda.synchronize()   # (the fill runs on torch's stream, the pipeline on the context's)
    ctx.set_restart_markers(restart)
    try:
        st = ctx.jpeg_decode_batch(jpegs, out, fs, threads=THREADS, frames_per_chunk=CHUNK, gpu_entropy=True)
    finally:
        ctx.set_restart_markers(False)
    got = out.cpu().numpy() if device else out
    assert np.array_equal(got, want)
    assert st.chunks == CHUNKS
    assert (st.entropy_ms_sum > 0) == (len(BAD_CHUNKS[bad]) > 0), st.entropy_ms_sum
