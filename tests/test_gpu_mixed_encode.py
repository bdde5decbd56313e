"""Mixed ENCODE batches on the GPU: hvc_encode_frames_mixed (frames of different geometry and tables in one launch of
k_encode_mixed) and hvc_jpeg_encode_batch_mixed (raw frames of different sizes, samplings and qualities in one call) against
the single-geometry entry points -- hvc_encode_frames, hvc_jpeg_encode -- and the model restatement, exactly."""
import numpy as np
import pytest

from oracle import orc

pytestmark = pytest.mark.gpu

FILL = 0x5A5A        # what stands between coefficient records, and in an output nobody may write
GAP = 40             # int16 elements between two coefficient records (80 bytes: the next record stays on 16)


@pytest.fixture()
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


def table(chroma, quality):
    return orc.quant_scale(orc.quant_chroma() if chroma else orc.quant_luma(), quality).astype(np.uint16)


def make_frame(planes, tables, seed, fill=None, pad=8):
    """planes: (blocks_w, blocks_h, qtab) each, pixel rows `pad` bytes wider than the plane, coefficient planes tight; tables:
    arrays of 64; fill(rows, cols) -> the pixels (default: seeded random bytes) -> dict(info, pixels (the record, noise between
    the rows' ends), want (the restatement's tight coefficient record))"""
    import video_coding_amd as hvc
    rng = np.random.Generator(np.random.PCG64(seed))
    info = hvc.hvc.JpegInfo()
    info.n_comp, info.n_qtabs = len(planes), len(tables)
    for t, q in enumerate(tables):
        for k in range(64):
            info.qtabs[t][k] = int(q[k])
    rec, want, co, po = [], [], 0, 0
    for i, (bw, bh, qt) in enumerate(planes):
        stride = bw * 8 + pad
        L = info.layout[i]
        L.blocks_w, L.blocks_h, L.qtab, L.coef_offset, L.plane_offset, L.stride = bw, bh, qt, co, po, stride
        if bw * bh:
            p = rng.integers(0, 256, size=(bh * 8, stride), dtype=np.uint8)
            if fill is not None:
                p[:, :bw * 8] = fill(bh * 8, bw * 8)
            rec.append(p.reshape(-1))
            want.append(orc.fdct_quant(rec[-1], tables[qt], bw, bh, stride=stride))
        co += bw * bh * 64
        po += stride * bh * 8
    info.coef_count, info.pixel_bytes = co, po
    return dict(info=info, planes=planes, tables=tables, pixels=np.concatenate(rec) if rec else np.zeros(0, np.uint8),
                want=np.concatenate(want) if want else np.zeros(0, np.int16))


def alone(ctx, fr):
    """hvc_encode_frames on that frame alone (host memory)"""
    L = fr["info"].layout
    specs = [dict(blocks_w=bw, blocks_h=bh, qtab=qt, coef_offset=L[i].coef_offset, plane_offset=L[i].plane_offset, stride=L[i].stride)
             for i, (bw, bh, qt) in enumerate(fr["planes"])]
    out = np.full(fr["want"].size, FILL, dtype=np.int16)
    ctx.encode_frames(fr["pixels"], fr["info"].pixel_bytes, np.stack(fr["tables"]), specs, 1, out, fr["info"].coef_count)
    return out


def place(frames, align=64):
    co, po, c, p = [], [], 0, 0
    for fr in frames:
        co.append(c)
        po.append(p)
        c += fr["want"].size + GAP
        p += -(-fr["pixels"].size // align) * align
    pixels = np.zeros(p + 8, dtype=np.uint8)
    for fr, off in zip(frames, po):
        pixels[off:off + fr["pixels"].size] = fr["pixels"]
    return co, po, pixels, np.full(c + 8, FILL, dtype=np.int16)


def run_mixed(ctx, frames, device):
    """the frames' pixel records 64 bytes apart at least, their coefficient records GAP elements of FILL apart -> the
    coefficient buffer and the offsets"""
    import torch
    co, po, pixels, coefs = place(frames)
    infos = [fr["info"] for fr in frames]
    if device:
        d_p, d_c = torch.from_numpy(pixels).cuda(), torch.from_numpy(coefs).cuda()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.encode_frames_mixed(d_p, po, infos, d_c, co)
        ctx.synchronize()
        ctx.reset_stream()
        coefs = d_c.cpu().numpy()
    else:
        ctx.encode_frames_mixed(pixels, po, infos, coefs, co)
    return coefs, co


def check_records(ctx, frames, coefs, co):
    end = 0
    for k, (fr, off) in enumerate(zip(frames, co)):
        assert (coefs[end:off] == FILL).all(), k                      # the gap between records is nobody's to write
        got = coefs[off:off + fr["want"].size]
        assert np.array_equal(got, fr["want"]), k                     # == the restatement (orc.fdct_quant)
        assert np.array_equal(got, alone(ctx, fr)), k                 # == hvc_encode_frames on that frame alone
        end = off + fr["want"].size
    assert (coefs[end:] == FILL).all()


@pytest.fixture(scope="module")
def shapes():
    ql, qc = table(0, 75), table(1, 75)
    return [
        make_frame([(1, 1, 0)], [ql], 11),                                    # one block
        make_frame([(8, 8, 0), (4, 4, 1), (4, 4, 1)], [ql, qc], 21),          # planes of 64 / 16 / 16 blocks
        make_frame([(9, 8, 0), (9, 8, 1), (9, 8, 1)], [ql, qc], 31),          # 72 blocks: a unit boundary
        make_frame([(1, 257, 0)], [qc], 41),                                  # bw = 1, a workgroup boundary
        make_frame([(66, 33, 0), (33, 33, 1), (33, 33, 1)], [ql, qc], 51),    # 4:2:2
    ]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_records_of_different_geometry(ctx, shapes, device, reverse):
    frames = shapes[::-1] if reverse else shapes
    coefs, co = run_mixed(ctx, frames, device)
    check_records(ctx, frames, coefs, co)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_pixel_extremes(ctx, device):
    """all 0, all 255, and a 0 / 255 checkerboard under a table of ones and under a table of 255s: the quantiser's extremes"""
    ones, top = np.ones(64, np.uint16), np.full(64, 255, np.uint16)
    board = lambda r, c: (((np.arange(r)[:, None] + np.arange(c)[None, :]) & 1) * 255).astype(np.uint8)
    planes = [(9, 8, 0), (3, 3, 1)]
    frames = [make_frame(planes, [table(0, 50), table(1, 50)], 1, fill=lambda r, c: np.zeros((r, c), np.uint8)),
              make_frame(planes, [table(0, 50), table(1, 50)], 2, fill=lambda r, c: np.full((r, c), 255, np.uint8)),
              make_frame(planes, [ones, top], 3, fill=board),
              make_frame(planes, [top, ones], 4, fill=board),
              make_frame(planes, [ones, top], 5)]
    coefs, co = run_mixed(ctx, frames, device)
    check_records(ctx, frames, coefs, co)
    luma = 72 * 64                                                            # (the same board divided by 4 and by 1020)
    assert np.abs(frames[2]["want"][:luma]).max() > 255 * np.abs(frames[3]["want"][:luma]).max() / 2 > 0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_adjacent_frames_with_different_tables(ctx, device):
    """qualities 20, 75 and 95 side by side, then the first tables again: a wrong table index changes bytes"""
    planes = [(7, 5, 0), (5, 3, 1)]
    frames = [make_frame(planes, [table(0, q), table(1, q)], 100 + q) for q in (20, 75, 95)]
    frames.append(make_frame(planes, [table(0, 20), table(1, 20)], 400))
    coefs, co = run_mixed(ctx, frames, device)
    check_records(ctx, frames, coefs, co)
    same = make_frame(planes, [table(0, 95), table(1, 95)], 120)              # the pixels of the quality 20 frame
    assert not np.array_equal(frames[0]["want"], same["want"])


def test_what_is_refused_leaves_the_output_untouched(ctx):
    import torch
    import video_coding_amd as hvc
    ok = make_frame([(3, 2, 0)], [table(0, 75)], 7)
    q300 = table(0, 50).copy()
    q300[5] = 300
    cases = [(make_frame([(3, 2, 0)], [table(0, 75)], 8), -1, "hardcaml"),
             (make_frame([(3, 2, 0), (2, 2, 1)], [table(0, 75), q300], 9), -5, None),          # HVC_E_RANGE
             (make_frame([(3, 2, 0), (0, 2, 0)], [table(0, 75)], 10), -1, None),               # a zero-size component
             (make_frame([(3, 2, 0), (2, 0, 0)], [table(0, 75)], 11), -1, None)]
    for bad, code, arith in cases:
        frames = [ok, bad]
        co, po, pixels, coefs = place(frames)
        infos = [fr["info"] for fr in frames]
        d_p, d_c = torch.from_numpy(pixels).cuda(), torch.from_numpy(coefs).cuda()
        if arith:
            ctx.set_encode_arithmetic(arith)
        for p, c in ((pixels, coefs), (d_p, d_c)):
            with pytest.raises(hvc.HvcError) as e:
                ctx.encode_frames_mixed(p, po, infos, c, co)
            assert e.value.code == code
        ctx.synchronize()
        ctx.set_encode_arithmetic("model")
        assert (coefs == FILL).all() and (d_c.cpu().numpy() == FILL).all()
    # the same calls go through once the reason is gone
    co, po, pixels, coefs = place([ok])
    ctx.encode_frames_mixed(pixels, po, [ok["info"]], coefs, co)
    assert np.array_equal(coefs[:ok["want"].size], ok["want"])


def test_an_empty_set_launches_nothing(ctx):
    """... which the profiling ring shows: a device-memory call takes an entry of it for k_encode_mixed, an empty one takes none"""
    import torch
    import video_coding_amd as hvc
    ctx.set_profiling(True)
    ctx.encode_frames_mixed(np.zeros(8, np.uint8), [], [], np.zeros(8, np.int16), [])
    d_p, d_c = torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.zeros(4096, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.encode_frames_mixed(d_p, [], [], d_c, [])
    with pytest.raises(hvc.HvcError):
        ctx.last_kernel_ms()                                                  # no profiled call yet
    fr = make_frame([(3, 2, 0)], [table(0, 75)], 7, pad=0)
    ctx.encode_frames_mixed(d_p, [0], [fr["info"]], d_c, [0])
    ctx.synchronize()
    assert ctx.last_kernel_ms() > 0


# ---------------------------------------------------------------------------
# files

# (width, height, chroma, quality); the 4:2:0 frame of width 16 k + 1 in the middle is the model's refusal
FRAMES = [(8, 8, 444, 1), (2, 2, 420, 50), (17, 9, 444, 100), (33, 16, 420, 75), (64, 64, 420, 1), (72, 64, 444, 50),
          (520, 264, 422, 100)]
BAD = 3


def raw_frame(k, w, h, chroma):
    """a seeded frame with structure and noise, tight Y, U, V"""
    rng = np.random.Generator(np.random.PCG64(900 + k))
    cw, ch = orc.chroma_dims(chroma, w, h)
    out = []
    for pw, ph in ((w, h), (cw, ch), (cw, ch)):
        yy, xx = np.mgrid[0:ph, 0:pw]
        p = 128 + 90 * np.sin(xx / 5.0 + k) * np.cos(yy / 7.0) + rng.integers(-30, 31, size=(ph, pw))
        out.append(np.clip(p, 0, 255).astype(np.uint8).reshape(-1))
    return np.concatenate(out)


@pytest.fixture(scope="module")
def raws():
    return [raw_frame(k, w, h, c) for k, (w, h, c, _) in enumerate(FRAMES)]


def singles(ctx, raws):
    """Context.jpeg_encode of every good frame alone, under the context's settings"""
    out = []
    for k, ((w, h, c, q), raw) in enumerate(zip(FRAMES, raws)):
        out.append(None if k == BAD else ctx.jpeg_encode(*orc.split_yuv(raw.tobytes(), w, h, c), w, h, c, q))
    return out


def check_files(results, want):
    for k, (status, jpg, size) in enumerate(results):
        if k == BAD:
            assert status == -1 and jpg is None
            continue
        assert status == 0, k
        assert jpg == want[k], k
        assert size == len(want[k])


@pytest.mark.parametrize("restart", [0, 1, 3])
@pytest.mark.parametrize("tables", ["default", "optimised"])
def test_files_equal_the_single_frame_encoder(ctx, raws, tables, restart):
    ctx.set_huffman_tables(tables)
    ctx.set_restart_interval(restart)
    want = singles(ctx, raws)
    outs = [np.full(len(w) + 64 if w else 64, 0xA5, dtype=np.uint8) for w in want]
    results = ctx.jpeg_encode_batch_mixed(raws, FRAMES, threads=4, outs=outs)
    check_files(results, want)
    assert (outs[BAD] == 0xA5).all()                                          # the refused frame's jpegs[f] is untouched
    st = ctx.last_batch_stats
    assert st.chunks == 1 and st.frames_per_chunk == len(FRAMES) - 1 and st.threads == 4
    if tables == "default" and restart == 0:
        # ... and the files go back through the mixed decoder, every one of them
        back = ctx.jpeg_decode_batch_mixed([r[1] for k, r in enumerate(results) if k != BAD])
        assert [b[0] for b in back] == [0] * (len(FRAMES) - 1)


@pytest.mark.parametrize("threads", [1, 4])
def test_one_frame_per_chunk_reuses_the_ring(ctx, raws, threads):
    """chunk_bytes below every frame's record: a chunk per frame, six chunks through a ring of three slots"""
    want = singles(ctx, raws)
    results = ctx.jpeg_encode_batch_mixed(raws, FRAMES, threads=threads, chunk_bytes=64)
    check_files(results, want)
    st = ctx.last_batch_stats
    assert st.chunks == len(FRAMES) - 1 > 3 and st.frames_per_chunk == 1 and st.threads == threads
    # twice through the same context, with two frames per chunk where they fit
    results = ctx.jpeg_encode_batch_mixed(raws[::-1], FRAMES[::-1], threads=threads, chunk_bytes=4096)
    check_files(results[::-1], want)
    assert 1 < ctx.last_batch_stats.chunks < len(FRAMES) - 1


def test_a_capacity_one_byte_short(ctx, raws):
    want = singles(ctx, raws)
    short = 4
    caps = [len(w) if w else 8 for w in want]
    caps[short] -= 1
    outs = [np.full(c + 8, 0xA5, dtype=np.uint8) for c in caps]
    results = ctx.jpeg_encode_batch_mixed(raws, FRAMES, threads=4, caps=caps, outs=outs)
    assert results[short][0] == -1 and results[short][2] == len(want[short])   # HVC_E_INVALID_ARG and the size it needs
    assert (outs[short] == 0xA5).all()
    for k, (status, jpg, size) in enumerate(results):
        if k not in (BAD, short):
            assert status == 0 and jpg == want[k], k                           # its neighbours are right
    assert results[BAD][0] == -1


def test_hardcaml_arithmetic_is_refused(ctx, raws):
    import video_coding_amd as hvc
    ctx.set_encode_arithmetic("hardcaml")
    outs = [np.full(70000, 0xA5, dtype=np.uint8) for _ in FRAMES]
    with pytest.raises(hvc.HvcError) as e:
        ctx.jpeg_encode_batch_mixed(raws, FRAMES, outs=outs)
    assert e.value.code == -1 and all((o == 0xA5).all() for o in outs)


def test_command_line(tmp_path):
    """`model encode frames` into a directory == `model encode frame` per input; the refused frame is named and skipped"""
    from video_coding_amd.__main__ import main
    args, names = [], []
    for k, (w, h, c, _) in enumerate(FRAMES):
        if c != 420 and k != 0:
            continue
        w, h = (w, h) if c == 420 else (24, 40)
        p = tmp_path / ("in%d.yuv" % k)
        p.write_bytes(raw_frame(k, w, h, 420).tobytes())
        args += [str(p), "%dx%d" % (w, h)]
        names.append((k, p, w, h))
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as e:                                       # (the refused frame: exit status 1)
        main(["model", "encode", "frames", str(out)] + args + ["-quality", "60", "-huffman", "optimised", "-restart-interval", "2"])
    assert e.value.code == 1
    for k, p, w, h in names:
        got = out / ("in%d.jpg" % k)
        if k == BAD:
            assert not got.exists()
            continue
        one = tmp_path / ("one%d.jpg" % k)
        main(["model", "encode", "frame", str(p), "%dx%d" % (w, h), str(one), "-quality", "60", "-huffman", "optimised",
              "-restart-interval", "2"])
        assert got.read_bytes() == one.read_bytes(), k
