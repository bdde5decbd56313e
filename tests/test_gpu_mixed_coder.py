"""hvc_jpeg_encode_batch_mixed_gpu: raw frames of different sizes, samplings and qualities to files in one call with the
Huffman coder on the GPU too (the mixed coder, csrc/hvc_huff_mixed.hip) -- against hvc_jpeg_encode_batch_mixed (the host coder)
and Context.jpeg_encode per frame: the same bytes, the same status, the same size, whoever coded the file."""
import numpy as np
import pytest

from test_gpu_mixed_encode import BAD, FRAMES, check_files, raw_frame, singles

pytestmark = pytest.mark.gpu

GOOD = len(FRAMES) - 1


@pytest.fixture()
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def raws():
    return [raw_frame(k, w, h, c) for k, (w, h, c, _) in enumerate(FRAMES)]


@pytest.mark.parametrize("chunk_bytes", [0, 4096, 64], ids=["one_chunk", "several", "one_per_file"])
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("tables", ["default", "optimised"])
def test_files_equal_the_host_coders(ctx, raws, tables, threads, chunk_bytes):
    ctx.set_huffman_tables(tables)
    want = singles(ctx, raws)
    host = ctx.jpeg_encode_batch_mixed(raws, FRAMES, threads=threads, chunk_bytes=chunk_bytes)
    outs = [np.full(len(w) + 64 if w else 64, 0xA5, dtype=np.uint8) for w in want]
    got = ctx.jpeg_encode_batch_mixed_gpu(raws, FRAMES, threads=threads, chunk_bytes=chunk_bytes, outs=outs)
    assert got == host                                            # every result tuple
    check_files(got, want)                                        # == Context.jpeg_encode per frame
    assert (outs[BAD] == 0xA5).all()
    assert ctx.last_mixed_coder_files() == (GOOD, 0)
    st = ctx.last_batch_stats
    assert st.threads == threads and st.chunks == {0: 1, 64: GOOD}.get(chunk_bytes, st.chunks) and 1 <= st.chunks <= GOOD
    if chunk_bytes == 4096:
        assert 1 < st.chunks < GOOD
    # the segment bytes that came down: the files without their headers and EOI
    assert 0 < st.coef_bytes < sum(len(w) for w in want if w)
    if tables == "default" and threads == 4 and chunk_bytes == 0:
        back = ctx.jpeg_decode_batch_mixed([r[1] for k, r in enumerate(got) if k != BAD])
        assert [b[0] for b in back] == [0] * GOOD


@pytest.mark.parametrize("tables", ["default", "optimised"])
def test_a_restart_interval_goes_to_the_host_coder(ctx, raws, tables):
    """the hand-back path: restart intervals are not in the mixed GPU coder, so every file is the host coder's, in one pass"""
    ctx.set_huffman_tables(tables)
    ctx.set_restart_interval(3)
    want = singles(ctx, raws)
    got = ctx.jpeg_encode_batch_mixed_gpu(raws, FRAMES, threads=4)
    assert got == ctx.jpeg_encode_batch_mixed(raws, FRAMES, threads=4)
    check_files(got, want)
    assert ctx.last_mixed_coder_files() == (0, GOOD)
    ctx.set_restart_interval(0)
    ctx.jpeg_encode_batch_mixed_gpu(raws, FRAMES, threads=4)
    assert ctx.last_mixed_coder_files() == (GOOD, 0)


def test_a_capacity_one_byte_short(ctx, raws):
    want = singles(ctx, raws)
    short = 4
    caps = [len(w) if w else 8 for w in want]
    caps[short] -= 1
    outs = [np.full(c + 8, 0xA5, dtype=np.uint8) for c in caps]
    got = ctx.jpeg_encode_batch_mixed_gpu(raws, FRAMES, threads=4, caps=caps, outs=outs)
    assert got[short][0] == -1 and got[short][2] == len(want[short])           # HVC_E_INVALID_ARG and the size it needs
    assert (outs[short] == 0xA5).all()
    assert got == ctx.jpeg_encode_batch_mixed(raws, FRAMES, threads=4, caps=caps)
    for k, (status, jpg, size) in enumerate(got):
        if k not in (BAD, short):
            assert status == 0 and jpg == want[k], k
    assert got[BAD][0] == -1


def test_failing_files_across_ring_reuse(ctx, raws):
    """one chunk per file -- more chunks than the ring has slots -- with a capacity one byte short and the refused frame in
    the middle: both pipelines give the same results over the same chunks and leave the same bytes in every buffer"""
    want = singles(ctx, raws)
    short = 5
    caps = [len(w) if w else 8 for w in want]
    caps[short] -= 1
    res, chunks, bufs = {}, {}, {}
    for name, call in (("host", ctx.jpeg_encode_batch_mixed), ("gpu", ctx.jpeg_encode_batch_mixed_gpu)):
        bufs[name] = [np.full(c + 8, 0xA5, dtype=np.uint8) for c in caps]
        res[name] = call(raws, FRAMES, threads=4, chunk_bytes=64, caps=caps, outs=bufs[name])
        chunks[name] = ctx.last_batch_stats.chunks
    assert res["gpu"] == res["host"] and chunks["gpu"] == chunks["host"] == GOOD
    assert ctx.last_mixed_coder_files() == (GOOD, 0)
    for k, (status, jpg, size) in enumerate(res["gpu"]):
        assert np.array_equal(bufs["gpu"][k], bufs["host"][k]), k
        if k in (BAD, short):
            assert status == -1 and (bufs["gpu"][k] == 0xA5).all(), k
        else:
            assert status == 0 and jpg == want[k] and (bufs["gpu"][k][size:] == 0xA5).all(), k
    assert res["gpu"][short][2] == len(want[short])


def test_hardcaml_arithmetic_is_refused(ctx, raws):
    import video_coding_amd as hvc
    ctx.set_encode_arithmetic("hardcaml")
    outs = [np.full(70000, 0xA5, dtype=np.uint8) for _ in FRAMES]
    with pytest.raises(hvc.HvcError) as e:
        ctx.jpeg_encode_batch_mixed_gpu(raws, FRAMES, outs=outs)
    assert e.value.code == -1 and all((o == 0xA5).all() for o in outs)


def test_command_line(tmp_path):
    """`model encode frames ... -coder gpu` writes what `-coder host` writes"""
    from video_coding_amd.__main__ import main
    args = []
    for k, (w, h) in enumerate([(24, 40), (2, 2), (64, 64), (33, 16), (200, 72)]):
        p = tmp_path / ("in%d.yuv" % k)
        p.write_bytes(raw_frame(k, w, h, 420).tobytes())
        args += [str(p), "%dx%d" % (w, h)]
    for coder in ("gpu", "host"):
        with pytest.raises(SystemExit) as e:                                   # (the refused 33 x 16 frame: exit status 1)
            main(["model", "encode", "frames", str(tmp_path / coder)] + args + ["-quality", "90", "-huffman", "optimised", "-coder", coder])
        assert e.value.code == 1
    names = sorted(p.name for p in (tmp_path / "host").iterdir())
    assert names == ["in0.jpg", "in1.jpg", "in2.jpg", "in4.jpg"] == sorted(p.name for p in (tmp_path / "gpu").iterdir())
    for n in names:
        assert (tmp_path / "gpu" / n).read_bytes() == (tmp_path / "host" / n).read_bytes(), n
