"""Mixed encode batches from RGB images: hvc_rgb_to_yuv_mixed, hvc_encode_frames_mixed_rgb and hvc_jpeg_encode_batch_mixed_rgb[_gpu]
(k_rgb_to_ycc_mixed, csrc/hvc_mixed_rgb.hip) against what the single-image calls give on a second context -- hvc_rgb_to_yuv and
hvc_jpeg_encode_rgb per image -- and, for the planes, against tools/rgb_reference.py.  Every comparison is exact equality.

The geometries hit every boundary of the decomposition (tests/test_mixed_rgb_encode_plan.py checks the plan of the same set on
the CPU): one lane; exactly one unit, one lane short of it, one lane over it; groups == 1; a partial last column group; several
units with 17 column groups.  As one set in that order the unit count (22) is no multiple of 4, so the last workgroup has spare
units; the set runs again reversed."""
import os
import sys

import numpy as np
import pytest

from conftest import golden_bytes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import rgb_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
GEO = [(444, 1, 1), (422, 2, 1), (420, 2, 2), (420, 16, 64), (420, 24, 42), (444, 8, 65), (422, 40, 13), (444, 8, 3), (420, 6, 4),
       (422, 10, 3), (420, 18, 10), (420, 136, 66)]
QUALITY = [75, 1, 100, 50, 90, 20, 75, 100, 35, 60, 85, 95]
SPECS = [(w, h, s, q) for (s, w, h), q in zip(GEO, QUALITY)]


@pytest.fixture()
def ctx():
    from video_coding_amd import hvc
    c = hvc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def images():
    """seeded random RGB bytes, [h, w, 3], one per geometry"""
    rng = np.random.Generator(np.random.PCG64(20261019))
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _, w, h in GEO]


@pytest.fixture(scope="module")
def single():
    """the reference: hvc_rgb_to_yuv / hvc_jpeg_encode_rgb per image, on a context of its own; computed once per setting"""
    from video_coding_amd import hvc
    c = hvc.Context(0)
    cache = {}

    def files(images, specs, tables="default", restart=0):
        key = (tables, restart, tuple(specs), tuple(id(i) for i in images))
        if key not in cache:
            c.set_huffman_tables(tables)
            c.set_restart_interval(restart)
            out = []
            for im, (w, h, s, q) in zip(images, specs):
                try:
                    out.append(c.jpeg_encode_rgb(im, s, q))
                except hvc.HvcError as e:
                    out.append(e.code)
            cache[key] = out
        return cache[key]

    def planes(im, info, sampling):
        """hvc_rgb_to_yuv of one image into a zeroed padded record of info"""
        rec = np.zeros(info.pixel_bytes, dtype=np.uint8)
        c.rgb_to_yuv(im, im.shape[1], im.shape[0], sampling, rec, info.layout)
        return rec

    c.files, c.planes = files, planes
    yield c
    c.close()


def arrange(images, layout):
    return [np.ascontiguousarray(im.transpose(2, 0, 1)) if layout == "planar" else im for im in images]


def put_images(images, lay, layout):
    """the images at lay.rgb_offsets with rows lay.rgb_row_strides apart, FILL between them"""
    buf = np.full(lay.total_bytes + 8, FILL, dtype=np.uint8)
    for f, im in enumerate(images):
        h, w = im.shape[:2]
        rs, off = lay.rgb_row_strides[f], lay.rgb_offsets[f]
        rows = im.transpose(2, 0, 1).reshape(3 * h, w) if layout == "planar" else im.reshape(h, 3 * w)
        view = buf[off:off + rows.shape[0] * rs - (rs - rows.shape[1])]
        for y in range(rows.shape[0]):
            view[y * rs:y * rs + rows.shape[1]] = rows[y]
    return buf


def odd_infos(hvc, order):
    """raw planes at odd offsets with odd strides: the byte path of every store"""
    infos, offs, at = [], [], 1
    for s, w, h in order:
        info = hvc.JpegInfo()
        info.width, info.height, info.n_comp, info.n_qtabs = w, h, 3, 1
        cw, ch = (w if s == 444 else w // 2), (h // 2 if s == 420 else h)
        po = 0
        for i, (hs, vs) in enumerate({420: [(2, 2), (1, 1), (1, 1)], 422: [(2, 1), (1, 1), (1, 1)], 444: [(1, 1)] * 3}[s]):
            info.comp[i].hscale, info.comp[i].vscale = hs, vs
            pw, ph = (w, h) if i == 0 else (cw, ch)
            L = info.layout[i]
            L.stride = (pw + 2) | 1
            L.plane_offset = po
            po += L.stride * ph + 1
        info.pixel_bytes = po
        infos.append(info)
        offs.append(at)
        at += po + (0 if (at + po) % 2 else 1)       # the next record at an odd offset again
    return infos, offs, at


def want_planes(images, order, infos, offs, total):
    """FILL everywhere but each frame's own samples, which are tools/rgb_reference.py's"""
    want = np.full(total, FILL, dtype=np.uint8)
    for im, (s, w, h), info, off in zip(images, order, infos, offs):
        for i, p in enumerate(ref.rgb_to_planes(im, s)):
            L = info.layout[i]
            for y in range(p.shape[0]):
                at = off + L.plane_offset + y * L.stride
                want[at:at + p.shape[1]] = p[y]
    return want


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_rgb_to_yuv_mixed(ctx, single, images, reverse, layout, device):
    from video_coding_amd import hvc
    order = GEO[::-1] if reverse else GEO
    specs = SPECS[::-1] if reverse else SPECS
    ims = images[::-1] if reverse else images
    for row_align, placement in ((0, "records"), (8, "records"), (0, "odd"), (8, "odd")):
        lay = hvc.jpeg_encoder_mixed_rgb_layout(specs, layout, 1 if placement == "odd" else 0, row_align)
        assert list(lay.status[:len(specs)]) == [0] * len(specs)
        rgb = put_images(ims, lay, layout)
        if placement == "records":
            infos, offs, total = [lay.infos[f] for f in range(len(specs))], list(lay.pixel_offsets[:len(specs)]), lay.pixel_total + 64
        else:
            infos, offs, total = odd_infos(hvc, order)
        want = want_planes(ims, order, infos, offs, total)
        yuv = np.full(total, FILL, dtype=np.uint8)
        if device:
            import torch
            d_y, d_r = torch.from_numpy(yuv).cuda(), torch.from_numpy(rgb).cuda()
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx.rgb_to_yuv_mixed(d_y, offs, infos, d_r, lay.rgb_offsets, lay.rgb_row_strides, layout)
            ctx.synchronize()
            ctx.reset_stream()
            yuv = d_y.cpu().numpy()
        else:
            ctx.rgb_to_yuv_mixed(yuv, offs, infos, rgb, lay.rgb_offsets, lay.rgb_row_strides, layout)
        assert np.array_equal(yuv, want), (row_align, placement)                      # the whole buffer: FILL outside the samples
        if placement == "records" and row_align == 0 and layout == "interleaved":       # == hvc_rgb_to_yuv per image
            for f, (im, (s, w, h)) in enumerate(zip(ims, order)):
                one = single.planes(im, infos[f], s)
                for i in range(3):
                    L, pw, ph = infos[f].layout[i], (w if i == 0 or s == 444 else w // 2), (h if i == 0 or s != 420 else h // 2)
                    a = one[L.plane_offset:L.plane_offset + L.stride * ph].reshape(ph, L.stride)[:, :pw]
                    b = yuv[offs[f] + L.plane_offset:offs[f] + L.plane_offset + L.stride * ph].reshape(ph, L.stride)[:, :pw]
                    assert np.array_equal(a, b), (f, i)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_encode_frames_mixed_rgb(ctx, single, images, reverse, layout, device):
    """records == hvc_encode_frames_mixed of hvc_rgb_to_yuv into zeroed padded records; the gaps in coefs keep their fill"""
    from video_coding_amd import hvc
    specs = SPECS[::-1] if reverse else SPECS
    ims = images[::-1] if reverse else images
    n = len(specs)
    lay = hvc.jpeg_encoder_mixed_rgb_layout(specs, layout, 0, 8 if reverse else 0)
    rgb = put_images(ims, lay, layout)
    gap = 24                                                                            # int16 elements of fill between the records
    co = [lay.coef_offsets[f] + gap * (f + 1) for f in range(n)]
    infos = [lay.infos[f] for f in range(n)]
    pixels = np.zeros(lay.pixel_total + 64, dtype=np.uint8)
    for f, (im, (w, h, s, q)) in enumerate(zip(ims, specs)):
        pixels[lay.pixel_offsets[f]:lay.pixel_offsets[f] + infos[f].pixel_bytes] = single.planes(im, infos[f], s)
    want = np.full(lay.coef_total + gap * (n + 1), 0x5A5A, dtype=np.int16)
    single.encode_frames_mixed(pixels, lay.pixel_offsets, infos, want, co)
    coefs = np.full(want.size, 0x5A5A, dtype=np.int16)
    if device:
        import torch
        d_c, d_r = torch.from_numpy(coefs).cuda(), torch.from_numpy(rgb).cuda()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.encode_frames_mixed_rgb(d_r, lay.rgb_offsets, infos, d_c, co, lay.rgb_row_strides, layout)
        ctx.synchronize()
        ctx.reset_stream()
        coefs = d_c.cpu().numpy()
    else:
        ctx.encode_frames_mixed_rgb(rgb, lay.rgb_offsets, infos, coefs, co, lay.rgb_row_strides, layout)
    assert np.array_equal(coefs, want)
    end = 0
    for f in range(n):
        assert (coefs[end:co[f]] == 0x5A5A).all(), f
        end = co[f] + infos[f].coef_count
    # a set that is refused leaves nothing behind: an odd width under 4:2:0 in the last frame
    bad = hvc.jpeg_encoder_mixed_layout(specs[:-1] + [(7, 4, 420, 75)])
    before = coefs.copy()
    with pytest.raises(hvc.HvcError) as e:
        ctx.encode_frames_mixed_rgb(rgb, lay.rgb_offsets, bad.infos, coefs, co, lay.rgb_row_strides, layout)
    assert e.value.code == -1 and np.array_equal(coefs, before)


def check(got, want):
    assert len(got) == len(want)
    for k, ((status, jpg, size), w) in enumerate(zip(got, want)):
        if isinstance(w, int):
            assert status == w and jpg is None, k
        else:
            assert status == 0 and jpg == w and size == len(w), k


@pytest.mark.parametrize("coder", ["host", "gpu"])
@pytest.mark.parametrize("chunk_bytes,threads", [(0, 4), (4096, 1), (4096, 4)], ids=["one_chunk_t4", "chunks_t1", "chunks_t4"])
@pytest.mark.parametrize("tables", ["default", "optimised"])
@pytest.mark.parametrize("restart", [0, 3])
def test_files_equal_jpeg_encode_rgb(ctx, single, images, restart, tables, chunk_bytes, threads, coder):
    reverse = threads == 1
    layout = "planar" if chunk_bytes and threads == 4 else "interleaved"
    specs = SPECS[::-1] if reverse else SPECS
    ims = images[::-1] if reverse else images
    want = single.files(ims, specs, tables, restart)
    assert all(isinstance(w, bytes) for w in want)
    ctx.set_huffman_tables(tables)
    ctx.set_restart_interval(restart)
    got = ctx.jpeg_encode_batch_mixed_rgb(arrange(ims, layout), specs, threads=threads, chunk_bytes=chunk_bytes, layout=layout, coder=coder)
    check(got, want)
    st = ctx.last_batch_stats
    assert st.threads == threads and (st.chunks >= 3 if chunk_bytes else st.chunks >= 1)
    if coder == "gpu":
        g, h = ctx.last_mixed_coder_files()
        assert g + h == len(specs) and (g == 0 if restart else h == 0)
        if chunk_bytes and not restart:
            assert st.chunks >= 3


def test_row_strides_and_the_same_chunks_as_the_yuv_call(ctx, single, images):
    """images with padded rows (rgb_row_strides), and the chunk count of the YUV call over the same infos"""
    from video_coding_amd import hvc
    want = single.files(images, SPECS)
    lay = hvc.jpeg_encoder_mixed_rgb_layout(SPECS, "interleaved", 0, 8)
    padded = []
    for f, im in enumerate(images):
        h, w = im.shape[:2]
        a = np.full((h, lay.rgb_row_strides[f]), FILL, dtype=np.uint8)
        a[:, :3 * w] = im.reshape(h, 3 * w)
        padded.append(a)
    for coder in ("host", "gpu"):
        got = ctx.jpeg_encode_batch_mixed_rgb(padded, enc_layout=lay, rgb_row_strides=lay.rgb_row_strides, chunk_bytes=4096, coder=coder)
        check(got, want)
        chunks = ctx.last_batch_stats.chunks
        yuv = [np.concatenate([p.reshape(-1) for p in ref.rgb_to_planes(im, s)]) for im, (s, _, _) in zip(images, GEO)]
        ctx.jpeg_encode_batch_mixed(yuv, layout=hvc.jpeg_encoder_mixed_layout(SPECS), chunk_bytes=4096, coder=coder)
        assert ctx.last_batch_stats.chunks == chunks


@pytest.mark.parametrize("coder", ["host", "gpu"])
def test_per_file_results(ctx, single, images, coder):
    """an odd-size image inside the set, a frame refused before the call and a capacity one byte short: each its documented
    status / size, jpegs[f] untouched, the neighbours unaffected"""
    from video_coding_amd import hvc
    rng = np.random.Generator(np.random.PCG64(7))
    specs = SPECS[:4] + [(7, 4, 420, 75)] + SPECS[4:8] + [(8, 8, 411, 75)] + SPECS[8:]            # odd width; an unknown chroma
    ims = images[:4] + [rng.integers(0, 256, (4, 7, 3), dtype=np.uint8)] + images[4:8] + [np.zeros((8, 8, 3), np.uint8)] + images[8:]
    odd, refused, short = 4, 9, 6
    want = single.files(ims, specs)
    assert want[odd] == -1 and want[refused] == -1
    # the layout call gives the odd image the status hvc_jpeg_encode_rgb gives it; hvc_jpeg_encoder_mixed_layout does not know the
    # rule, so with its infos the batch call itself must refuse the image
    rgb_lay, yuv_lay = hvc.jpeg_encoder_mixed_rgb_layout(specs), hvc.jpeg_encoder_mixed_layout(specs)
    assert rgb_lay.status[odd] == -1 and yuv_lay.status[odd] == 0 and yuv_lay.status[refused] == -1
    for lay in (rgb_lay, yuv_lay):
        caps = [len(w) if isinstance(w, bytes) else 64 for w in want]
        caps[short] -= 1
        outs = [np.full(c + 8, FILL, dtype=np.uint8) for c in caps]
        got = ctx.jpeg_encode_batch_mixed_rgb(ims, enc_layout=lay, threads=4, chunk_bytes=4096, caps=caps, outs=outs, coder=coder)
        assert got[odd][0] == -1 and got[odd][2] == 0 and (outs[odd] == FILL).all()
        assert got[refused][0] == -1 and got[refused][2] == 0 and (outs[refused] == FILL).all()
        assert got[short][0] == -1 and got[short][2] == len(want[short]) and (outs[short] == FILL).all()   # the size it needs
        for k, (status, jpg, size) in enumerate(got):
            if k not in (odd, refused, short):
                assert status == 0 and jpg == want[k], k
        if coder == "gpu":
            assert sum(ctx.last_mixed_coder_files()) == len(specs) - 2


def test_hardcaml_encode_arithmetic_is_refused(ctx, images):
    from video_coding_amd import hvc
    ctx.set_encode_arithmetic("hardcaml")
    lay = hvc.jpeg_encoder_mixed_rgb_layout(SPECS)
    for coder in ("host", "gpu"):
        outs = [np.full(70000, FILL, dtype=np.uint8) for _ in SPECS]
        with pytest.raises(hvc.HvcError) as e:
            ctx.jpeg_encode_batch_mixed_rgb(images, enc_layout=lay, outs=outs, coder=coder)
        assert e.value.code == -1 and all((o == FILL).all() for o in outs)
    coefs = np.full(lay.coef_total + 8, 0x5A5A, dtype=np.int16)
    with pytest.raises(hvc.HvcError) as e:
        ctx.encode_frames_mixed_rgb(put_images(images, lay, "interleaved"), lay.rgb_offsets, lay.infos, coefs, lay.coef_offsets)
    assert e.value.code == -1 and (coefs == 0x5A5A).all()


def test_round_trip_of_the_golden_files(ctx, single):
    """mixed decode to RGB, the images cropped to even sizes, mixed encode from RGB: the files are jpeg_encode_rgb's, and they
    decode (jpeg_decode_rgb) to images of those sizes"""
    files = [golden_bytes("mini.jpg"), golden_bytes("Mouse480.jpg")]
    decoded = ctx.jpeg_decode_batch_mixed_rgb(files)
    assert [d[0] for d in decoded] == [0, 0]
    ims = [np.ascontiguousarray(d[2][:d[2].shape[0] & ~1, :d[2].shape[1] & ~1]) for d in decoded]
    specs = [(im.shape[1], im.shape[0], 420, 75) for im in ims]
    want = single.files(ims, specs)
    for coder in ("host", "gpu"):
        got = ctx.jpeg_encode_batch_mixed_rgb(ims, specs, coder=coder)
        check(got, want)
    for (status, jpg, _), im in zip(got, ims):
        info, back = ctx.jpeg_decode_rgb(jpg)
        assert (info.width, info.height) == (im.shape[1], im.shape[0]) and back.shape == im.shape
        assert np.array_equal(back, single.jpeg_decode_rgb(jpg)[1])


def test_command_line(tmp_path, single, images):
    """`model encode frames ... -rgb` writes the files of jpeg_encode_rgb, with either coder"""
    from video_coding_amd.__main__ import main
    args, picked = [], [3, 8, 11, 4]
    for k in picked:
        p = tmp_path / ("in%d.ppm" % k)
        ref.write_ppm(str(p), images[k])
        args += [str(p), "%dx%d" % (GEO[k][1], GEO[k][2])]
    odd = tmp_path / "odd.ppm"
    ref.write_ppm(str(odd), np.zeros((4, 7, 3), np.uint8))
    want = single.files([images[k] for k in picked], [(GEO[k][1], GEO[k][2], 420, 90) for k in picked], "optimised", 0)
    for coder in ("gpu", "host"):
        with pytest.raises(SystemExit) as e:                                   # (the refused 7 x 4 image: exit status 1)
            main(["model", "encode", "frames", str(tmp_path / coder)] + args + [str(odd), "7x4", "-rgb", "-quality", "90", "-huffman", "optimised",
                                                                                 "-coder", coder])
        assert e.value.code == 1
        assert sorted(p.name for p in (tmp_path / coder).iterdir()) == sorted("in%d.jpg" % k for k in picked)
        for k, w in zip(picked, want):
            assert (tmp_path / coder / ("in%d.jpg" % k)).read_bytes() == w, k
    with pytest.raises(SystemExit) as e:                                       # a size that is not the PPM's own
        main(["model", "encode", "frames", str(tmp_path / "x"), args[0], "18x64", "-rgb"])
    assert e.value.code not in (0, None)
