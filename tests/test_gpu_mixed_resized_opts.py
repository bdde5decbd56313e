"""hvc_jpeg_decode_batch_mixed_resized_opts on the GPU: files of any geometry decoded (at 1 / scale_denom), converted to RGB and a
window of each taken to the size the caller names -- mirrored or not, as bytes or as the float16 tensor a model reads -- in one
call.  Every good file's record must equal tools/resize_reference.py resize_box (Pillow's Image.resize(box=...), bit for bit)
applied to what hvc_jpeg_decode_rgb / hvc_jpeg_decode_scaled_rgb gives for that file alone, then apply_lut; under the mixed
libjpeg arithmetic the records must be Pillow's own (tests/golden/resize_box_pins.json).  Buffers are compared whole over a
fill of 0xA5."""
import json
import os
import pathlib
import sys

import numpy as np
import pytest

import resize_box_cases as bc
from conftest import GOLDEN, golden_bytes
from test_gpu_mixed_resized import FILTERS, alone, ctx, file_set, host, hvc  # noqa: F401  (ctx, file_set, hvc: fixtures)
from test_host_entropy import unusual_sampling_file
from test_mixed_rgb_plan import FACTORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_resize_box_pins as mk  # noqa: E402
import resize_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
KINDS = ("fraction", "integer", "none", "left", "thin", "bottom", "whole", "top", "right")


def options(ctx_, files, codes, scale):
    """a box (in the coordinates of the image at 1 / scale) and a mirror flag for every file; the last good file's box leaves its
    image by one pixel, so that file gets HVC_E_INVALID_ARG as its own status"""
    boxes, mirror, want = [], [], list(codes)
    last_good = max(f for f, c in enumerate(codes) if c == 0)
    for f, (data, code) in enumerate(zip(files, codes)):
        mirror.append(f % 3 != 1)
        if code:
            boxes.append((0.0, 0.0, 1.0, 1.0))                   # (never looked at: the file has no image)
            continue
        h, w = alone(ctx_, data, scale).shape[:2]
        box = bc.boxes(w, h).get(KINDS[f % len(KINDS)])
        boxes.append(box if box is not None else (0.0, 0.0, float(w), float(h)))
        if f == last_good:
            boxes[-1] = (0.0, 0.0, float(w + 1), float(h))
            want[f] = -1
    return boxes, mirror, want


_WANT = {}


def want_record(ctx_, data, scale, W, H, filt, box, mirror, layout, lut):
    """the file's record as raw bytes"""
    key = (data, scale, W, H, filt, box, mirror)
    if key not in _WANT:
        _WANT[key] = rr.resize_box(alone(ctx_, data, scale), W, H, filt, box, mirror)
    img = _WANT[key]
    if lut is not None:
        img = rr.apply_lut(img, lut)
    return np.ascontiguousarray(img.transpose(2, 0, 1) if layout == "planar" else img).reshape(-1).view(np.uint8)


@pytest.mark.parametrize("dtype", [None, "float16"], ids=["uint8", "float16"])
@pytest.mark.parametrize("reader", ["host", "gpu"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("scale", [1, 2])
def test_files_to_one_tensor_under_options(ctx, hvc, file_set, scale, layout, reader, dtype):
    import torch
    files, codes = file_set
    n = len(files)
    device = (scale + (layout == "planar") + (reader == "gpu") + (dtype is not None)) % 2 == 1
    filt = FILTERS[(scale + (layout == "planar") + 2 * (reader == "gpu") + (dtype is not None)) % 3]
    W, H = 31, 17
    esz = 2 if dtype else 1
    lut = hvc.normalize_lut(*IMAGENET, dtype) if dtype else None
    boxes, mirror, want = options(ctx, files, codes, scale)
    frame = 3 * W * H * esz
    out = np.full(n * frame + 16, FILL, dtype=np.uint8)
    expect = out.copy()
    for f, data in enumerate(files):
        if want[f] == 0:
            expect[f * frame:(f + 1) * frame] = want_record(ctx, data, scale, W, H, filt, boxes[f], mirror[f], layout, lut)
    if device:
        out = torch.from_numpy(out).cuda()
    ctx.set_mixed_reader(reader)
    kw = dict(dtype=dtype, mean=IMAGENET[0], std=IMAGENET[1]) if dtype else {}
    status, tensor = ctx.jpeg_decode_batch_mixed_resized(files, size=(W, H), filter=filt, scale_denom=scale, layout=layout, device=device,
                                                         threads=2, chunk_bytes=40000, out=out, boxes=boxes, mirror=mirror, **kw)
    assert ctx.last_batch_stats.chunks >= 3
    assert status == want                                        # every status is the file's own, the box that leaves its image among them
    assert tuple(tensor.shape) == ((n, 3, H, W) if layout == "planar" else (n, H, W, 3))
    assert str(tensor.dtype).endswith(dtype or "uint8")
    assert np.array_equal(host(out), expect)                     # good files: the definition; failed files and the tail: the fill
    readers = ctx.last_mixed_reader_files()
    assert readers[0] > 0 if reader == "gpu" else readers[0] == 0


def test_without_options_it_is_the_call_as_it_was(ctx, hvc, file_set):
    """opts NULL and an all-zero block: byte for byte hvc_jpeg_decode_batch_mixed_resized, statuses included"""
    import ctypes as C
    files, codes = file_set
    lay = hvc.hvc.MixedLayout(files)
    n, (W, H) = len(files), (24, 16)
    ow, oh = (C.c_int * n)(*[W] * n), (C.c_int * n)(*[H] * n)
    offs = (C.c_size_t * n)(*[f * 3 * W * H for f in range(n)])
    outs = []
    for fn, opts in (("hvc_jpeg_decode_batch_mixed_resized", ()), ("hvc_jpeg_decode_batch_mixed_resized_opts", (None,)),
                     ("hvc_jpeg_decode_batch_mixed_resized_opts", (C.byref(hvc.hvc.ResizeOpts()),))):
        out = np.full(n * 3 * W * H + 8, FILL, dtype=np.uint8)
        status = (C.c_int * n)(*lay.status)
        st = hvc.hvc.BatchStats()
        r = getattr(hvc.lib(), fn)(ctx._h, lay.ptrs, lay.sizes, n, 2, 40000, 1, lay.infos, status, ow, oh, offs, None, out.ctypes.data, out.size, 0, 2, 0,
                                   C.byref(st), *opts)
        assert r == 0 and list(status) == codes
        outs.append(out)
    assert np.array_equal(outs[1], outs[0]) and np.array_equal(outs[2], outs[0])
    assert np.array_equal(outs[0][:3 * W * H].reshape(H, W, 3), rr.resize(alone(ctx, files[0], 1), W, H, "bicubic"))


def test_a_size_and_a_dtype_per_call(ctx, hvc, file_set):
    """sizes=: a view per file in the element type; bfloat16 through a table of the caller's own"""
    import torch
    files, codes = file_set
    good = [f for f, c in enumerate(codes) if c == 0][:5]
    datas = [files[f] for f in good]
    sizes = [(8 + 3 * k, 5 + 2 * k) for k in range(len(datas))]
    lut = hvc.normalize_lut((0.5, 0.5, 0.5), (0.25, 0.5, 1.0), "bfloat16")
    status, views = ctx.jpeg_decode_batch_mixed_resized(datas, sizes=sizes, filter="bilinear", device=True, threads=2, mirror=True, lut=lut, dtype=torch.bfloat16)
    assert status == [0] * len(datas)
    for data, (w, h), v in zip(datas, sizes, views):
        assert v.dtype == torch.bfloat16 and tuple(v.shape) == (h, w, 3)
        want = rr.apply_lut(rr.resize_box(alone(ctx, data, 1), w, h, "bilinear", None, True), lut)
        assert np.array_equal(v.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), want)


def test_refusals_leave_the_output_untouched(ctx, hvc, file_set):
    import ctypes as C
    files, _ = file_set
    out = np.full(len(files) * 3 * 8 * 8 * 2, FILL, dtype=np.uint8)
    lay = hvc.hvc.MixedLayout(files)
    n = len(files)
    for out_elem, table in ((1, True), (3, True), (2, False), (4, False)):
        o = hvc.hvc.ResizeOpts()
        lut = np.zeros((3, 256), np.uint32)
        o.out_elem, o.lut = out_elem, lut.ctypes.data if table else None
        status = (C.c_int * n)(*lay.status)
        ow = (C.c_int * n)(*[8] * n)
        offs = (C.c_size_t * n)(*[f * 3 * 64 * 2 for f in range(n)])
        r = hvc.lib().hvc_jpeg_decode_batch_mixed_resized_opts(ctx._h, lay.ptrs, lay.sizes, n, 2, 0, 1, lay.infos, status, ow, ow, offs, None, out.ctypes.data,
                                                               out.size, 0, 1, 0, None, C.byref(o))
        assert r == -1 and (out == FILL).all() and list(status) == list(lay.status), (out_elem, table)
    with pytest.raises(hvc.hvc.HvcError) as e:                   # a typed record outside the buffer: the cap counts bytes
        ctx.jpeg_decode_batch_mixed_resized(files, size=(8, 8), out=out[:len(files) * 3 * 64 * 2 - 1], dtype="float16")
    assert e.value.code == -1 and (out == FILL).all()
    ctx.set_mixed_arithmetic("libjpeg")                          # the libjpeg arithmetic decodes at full size only, options or not
    with pytest.raises(hvc.hvc.HvcError) as e:
        ctx.jpeg_decode_batch_mixed_resized(files, size=(8, 8), scale_denom=2, out=out, mirror=True)
    assert e.value.code == -1 and (out == FILL).all()


# ---- Pillow's own pixels ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(ROOT, "tests", "golden", "resize_box_pins.json")) as f:
        return json.load(f)["libjpeg_sha256"]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("reader", ["host", "gpu"])
def test_under_the_libjpeg_arithmetic_the_records_are_pillows(ctx, pins, reader, device):
    """hvc_set_mixed_arithmetic(HVC_ARITH_LIBJPEG), scale 1: Image.open(f).convert("RGB").resize((W, H), filter, box=box) and its
    FLIP_LEFT_RIGHT, by the stored hashes of Pillow's output"""
    ctx.set_mixed_arithmetic("libjpeg")
    ctx.set_mixed_reader(reader)
    cases = mk.golden_cases()
    assert set(pins) == {c[0] for c in cases}
    calls = {}
    for c in cases:
        calls.setdefault((c[2], c[3], c[4]), []).append(c)
    assert len(calls) == 6
    for k, ((W, H, filt), group) in enumerate(sorted(calls.items())):
        layout = "planar" if k % 2 else "interleaved"
        files = [golden_bytes(c[1]) for c in group]
        status, tensor = ctx.jpeg_decode_batch_mixed_resized(files, size=(W, H), filter=filt, layout=layout, device=device, threads=2, chunk_bytes=40000,
                                                             boxes=[c[5] for c in group], mirror=[c[6] for c in group])
        assert status == [0] * len(files)
        got = host(tensor)
        for f, c in enumerate(group):
            img = got[f].transpose(1, 2, 0) if layout == "planar" else got[f]
            assert bc.sha256(img) == pins[c[0]], c[0]


# ---- the command line -------------------------------------------------------------------------------------------------
def test_cli_box_and_mirror_write_what_the_python_call_gives(tmp_path, ctx):
    from video_coding_amd.__main__ import main
    golden = pathlib.Path(GOLDEN)
    third = tmp_path / "third.jpg"
    third.write_bytes(unusual_sampling_file(FACTORS[422], 97, 51, 4)[0])
    ins = [golden / "mini.jpg", golden / "Mouse480.jpg", third]
    datas = [p.read_bytes() for p in ins]
    box = (3.5, 2.25, 40.0, 30.5)
    for flags, kw, scale, filt in ((["-box", "3.5,2.25,40,30.5", "-mirror"], dict(boxes=box, mirror=True), 1, "bilinear"),
                                   (["-box", "3.5,2.25,40,30.5", "-filter", "bicubic"], dict(boxes=box), 1, "bicubic"),
                                   (["-mirror", "-scale", "2", "-reader", "gpu"], dict(mirror=True), 2, "bilinear")):
        W, H = 31, 17
        out = tmp_path / ("out%d" % len(flags))
        main(["model", "decode", "frames", str(out)] + [str(p) for p in ins] + ["-rgb", "-resize", "31x17"] + flags)
        status, tensor = ctx.jpeg_decode_batch_mixed_resized(datas, size=(W, H), filter=filt, scale_denom=scale, **kw)
        assert status == [0, 0, 0]
        for f, p in enumerate(ins):
            assert (out / (p.stem + ".ppm")).read_bytes() == b"P6\n%d %d\n255\n" % (W, H) + tensor[f].tobytes(), (flags, p)
            want = rr.resize_box(alone(ctx, datas[f], scale), W, H, filt, kw.get("boxes"), bool(kw.get("mirror")))
            assert np.array_equal(tensor[f], want), (flags, p)
    with pytest.raises(SystemExit):
        main(["model", "decode", "frames", str(tmp_path / "o"), str(ins[0]), "-rgb", "-box", "0,0,8,8"])   # -box belongs to -resize
