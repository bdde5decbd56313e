"""Mixed batches resized on the GPU: hvc_jpeg_decode_batch_mixed_resized -- files of any geometry decoded (at 1 / scale_denom),
converted to RGB and taken to the size the caller names, in one call, one tensor out.  Every good file's record must equal
tools/resize_reference.py (Pillow's Image.resize, bit for bit) applied to what hvc_jpeg_decode_rgb / hvc_jpeg_decode_scaled_rgb
gives for that file alone; buffers are compared whole over a fill of 0xA5."""
import os
import pathlib
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden_bytes
from test_host_entropy import unusual_sampling_file
from test_mixed_rgb_plan import FACTORS, UNCONVERTIBLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import resize_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5
FILTERS = ("box", "bilinear", "bicubic")


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd
    return video_coding_amd


@pytest.fixture()
def ctx(hvc):
    c = hvc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def file_set(hvc):
    """(files, the status each must get): the golden files, writer-made files of 4:2:0 / 4:2:2 / 4:4:4 / grey at odd sizes, and
    in the middle a file cut in its header, one cut in its scan, a SOF2 file and a 4:1:1 file"""
    mini, mouse = golden_bytes("mini.jpg"), golden_bytes("Mouse480.jpg")
    files, want = [mini, mouse], [0, 0]
    for (w, h) in ((70, 38), (97, 51)):
        for kind in (420, 422, 444, 400):
            files.append(unusual_sampling_file(FACTORS[kind], w, h, 3000 + kind + w)[0])
            want.append(0)
    info = hvc.hvc.jpeg_read_header(mouse)
    cut = mouse[:info.ecs_offset + 2000] + b"\xff\x00" * 64 + b"\xff\xd9"     # (one-bits follow the cut: no table has a code for them)
    with pytest.raises(hvc.hvc.HvcError) as e:
        hvc.hvc.jpeg_entropy_decode(cut)
    middle = [(mini[:100], -8), (cut, e.value.code), (mini.replace(b"\xff\xc0", b"\xff\xc2", 1), -9),
              (unusual_sampling_file(UNCONVERTIBLE[0], 45, 53, 77)[0], -1)]
    for k, (data, code) in enumerate(middle):
        files.insert(4 + 2 * k, data)
        want.insert(4 + 2 * k, code)
    for (w, h) in ((45, 53), (233, 9)):
        files.append(unusual_sampling_file(FACTORS[420], w, h, 4000 + w)[0])
        want.append(0)
    assert e.value.code != 0
    return files, want


_ALONE, _WANT = {}, {}


def alone(ctx, data, scale):
    """the file's RGB image by the single-file entry point, [h, w, 3]: computed once"""
    if (data, scale) not in _ALONE:
        _ALONE[data, scale] = ctx.jpeg_decode_rgb(data)[1] if scale == 1 else ctx.jpeg_decode_scaled_rgb(data, scale)[1]
    return _ALONE[data, scale]


def want_image(ctx, data, scale, W, H, filt, layout):
    key = (data, scale, W, H, filt)
    if key not in _WANT:
        _WANT[key] = rr.resize(alone(ctx, data, scale), W, H, filt)
    img = _WANT[key]
    return np.ascontiguousarray(img.transpose(2, 0, 1)) if layout == "planar" else img


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("reader", ["host", "gpu"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("scale", [1, 2])
def test_files_to_one_tensor(ctx, hvc, file_set, scale, layout, reader, device):
    import torch
    files, codes = file_set
    n = len(files)
    filt = FILTERS[(scale + (layout == "planar") + 2 * (reader == "gpu") + device) % 3]
    W, H = 31, 17
    out = np.full(n * 3 * W * H + 16, FILL, dtype=np.uint8)
    expect = out.copy()
    for f, (data, code) in enumerate(zip(files, codes)):
        if code == 0:
            expect[f * 3 * W * H:(f + 1) * 3 * W * H] = want_image(ctx, data, scale, W, H, filt, layout).reshape(-1)
    if device:
        out = torch.from_numpy(out).cuda()
    # what the RGB form of the same pipeline says about its readers, for the same files
    ctx.set_mixed_reader(reader)
    if scale == 1:
        ctx.jpeg_decode_batch_mixed_rgb(files, threads=2, chunk_bytes=40000)
    else:
        ctx.jpeg_decode_batch_mixed_scaled_rgb(files, scale, threads=2, chunk_bytes=40000)
    readers = ctx.last_mixed_reader_files()
    status, tensor = ctx.jpeg_decode_batch_mixed_resized(files, size=(W, H), filter=filt, scale_denom=scale, layout=layout, device=device,
                                                         threads=2, chunk_bytes=40000, out=out)
    assert ctx.last_batch_stats.chunks >= 3
    assert status == codes                                       # every status is the file's own
    assert tuple(tensor.shape) == ((n, 3, H, W) if layout == "planar" else (n, H, W, 3))
    assert np.array_equal(host(out), expect)                     # good files: the definition; failed files and the tail: the fill
    assert ctx.last_mixed_reader_files() == readers
    if reader == "gpu":
        assert readers[0] > 0
    else:
        assert readers[0] == 0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_size_per_file(ctx, hvc, file_set, device):
    """sizes=: aspect-preserving thumbnails, one view per file; enlarging, one axis the same and the same size among them"""
    files, codes = file_set
    sizes = []
    for f, data in enumerate(files):
        if codes[f] in (-8, -9):
            sizes.append((8, 8))
            continue
        info = hvc.hvc.jpeg_read_header(data)
        w, h = info.width, info.height
        sizes.append([(max(1, w * 24 // max(w, h)), max(1, h * 24 // max(w, h))), (w, h), (w, 8), (2 * w, h + 3)][f % 4] if w < 200 else (48, 32))
    status, views = ctx.jpeg_decode_batch_mixed_resized(files, sizes=sizes, filter="bicubic", device=device, threads=2, chunk_bytes=40000)
    assert status == codes
    for f, (data, code) in enumerate(zip(files, codes)):
        if code:
            assert views[f] is None
        else:
            assert np.array_equal(host(views[f]), want_image(ctx, data, 1, sizes[f][0], sizes[f][1], "bicubic", "interleaved")), f


def test_a_file_beyond_the_bounds_gets_its_own_status(ctx, hvc):
    """233 x 9 -> a row stride below the row, and a size of 0: the file's own status, its record untouched, nobody else stopped"""
    import ctypes as C
    files = [golden_bytes("mini.jpg"), unusual_sampling_file(FACTORS[420], 233, 9, 4233)[0], unusual_sampling_file(FACTORS[444], 70, 38, 3514)[0]]
    lay = hvc.hvc.jpeg_mixed_layout(files)
    n = len(files)
    out = np.full(3 * 4096, FILL, dtype=np.uint8)
    status = (C.c_int * n)(*lay.status)
    ow, oh = (C.c_int * n)(8, 0, 8), (C.c_int * n)(8, 8, 8)
    offs, strides = (C.c_size_t * n)(0, 4096, 8192), (C.c_size_t * n)(0, 0, 23)
    st = hvc.hvc.BatchStats()
    r = hvc.lib().hvc_jpeg_decode_batch_mixed_resized(ctx._h, lay.ptrs, lay.sizes, n, 2, 0, 1, lay.infos, status, ow, oh, offs, strides,
                                                      out.ctypes.data, out.size, 0, 1, 0, C.byref(st))
    assert r == 0 and list(status) == [0, -1, -1]
    assert np.array_equal(out[:192].reshape(8, 8, 3), rr.resize(alone(ctx, files[0], 1), 8, 8, "bilinear")) and (out[192:] == FILL).all()


def test_refusals_leave_the_output_untouched(ctx, hvc, file_set):
    files, _ = file_set
    out = np.full(len(files) * 3 * 8 * 8, FILL, dtype=np.uint8)
    for arith in ("libjpeg", "hardcaml"):                        # the mixed calls have no such form: this one inherits that
        ctx.set_arithmetic(arith)
        with pytest.raises(hvc.hvc.HvcError) as e:
            ctx.jpeg_decode_batch_mixed_resized(files, size=(8, 8), out=out)
        assert e.value.code == -1 and (out == FILL).all()
    ctx.set_arithmetic("model")
    for kw in (dict(filter=3), dict(layout=2), dict(scale_denom=3)):
        with pytest.raises(hvc.hvc.HvcError) as e:
            ctx.jpeg_decode_batch_mixed_resized(files, size=(8, 8), out=out, **kw)
        assert e.value.code == -1 and (out == FILL).all(), kw
    with pytest.raises(hvc.hvc.HvcError) as e:                   # a record outside the buffer
        ctx.jpeg_decode_batch_mixed_resized(files, size=(8, 8), out=out[:-1])
    assert e.value.code == -1 and (out == FILL).all()
    status, tensor = ctx.jpeg_decode_batch_mixed_resized(files[:2], size=(8, 8), out=out)     # and the context goes on
    assert status == [0, 0] and np.array_equal(tensor[0], rr.resize(alone(ctx, files[0], 1), 8, 8, "bilinear"))


def test_restart_markers_are_honoured_as_everywhere(ctx, hvc):
    from helpers import jpeg_optimised_tables
    from test_restart_intervals import QT, random_record
    # one file with DRI whose reading by the model (the first interval only) stays inside int16: tests/test_gpu_mixed_scaled.py
    rec, _ = random_record([(2, 2), (1, 1), (1, 1)], 200, 72, 9)
    blocks = rec.reshape(-1, 64).copy()
    rng = np.random.Generator(np.random.PCG64(1))
    blocks[:, 0] = 40
    blocks[rng.integers(0, len(blocks), size=30), 0] = rng.integers(-200, 200, size=30)
    blocks[rng.random(len(blocks)) < 0.6, 1:] = 0
    marked = jpeg_optimised_tables(200, 72, 420, QT, blocks.reshape(-1), restart_interval=5)
    seen = {}
    for honour in (False, True):
        ctx.set_restart_markers(honour)
        try:
            status, tensor = ctx.jpeg_decode_batch_mixed_resized([golden_bytes("mini.jpg"), marked], size=(50, 18), filter="box", threads=2)
            assert status == [0, 0]
            assert np.array_equal(tensor[1], rr.resize(ctx.jpeg_decode_rgb(marked)[1], 50, 18, "box"))   # the same setting, the file alone
            seen[honour] = tensor[1].copy()
        finally:
            ctx.set_restart_markers(False)
    assert not np.array_equal(seen[False], seen[True])


def test_cli_decode_frames_resize(tmp_path, ctx):
    from video_coding_amd.__main__ import main
    golden = pathlib.Path(GOLDEN)
    third = tmp_path / "third.jpg"
    third.write_bytes(unusual_sampling_file(FACTORS[422], 97, 51, 4)[0])
    ins = [golden / "mini.jpg", golden / "Mouse480.jpg", third]
    for flags, scale, filt in ((["-resize", "31x17"], 1, "bilinear"), (["-resize", "40x30", "-filter", "bicubic", "-scale", "2", "-reader", "gpu"], 2, "bicubic")):
        W, H = (int(v) for v in flags[1].split("x"))
        out = tmp_path / ("out%d" % scale)
        main(["model", "decode", "frames", str(out)] + [str(p) for p in ins] + ["-rgb"] + flags)
        for p in ins:
            want = want_image(ctx, p.read_bytes(), scale, W, H, filt, "interleaved")
            assert (out / (p.stem + ".ppm")).read_bytes() == b"P6\n%d %d\n255\n" % (W, H) + want.tobytes(), p
    with pytest.raises(SystemExit):
        main(["model", "decode", "frames", str(tmp_path / "o"), str(ins[0]), "-resize", "8x8"])       # -resize takes -rgb
