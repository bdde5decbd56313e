"""The single-file decode entry points (hvc_jpeg_decode, hvc_jpeg_decode_yuv444, hvc_jpeg_decode_rgb) on each of the four ways
a file can take through them, every result against the checker (oracle/orc.py; RGB: tools/rgb_reference.py over its planes):

  small      below 128 kB: the host reader, then the block stage
  speculated 128 kB and more: the GPU Huffman reader with the block stage enqueued behind it before its verdict is known
  refused    a large file the GPU reader hands back (truncated: "stream ends early") after the block stage was enqueued
             behind it: the host reader takes over, and the next call on the context is still exact
  wide_dc    a large file whose DC leaves int16: the GPU reader's DC pass refuses it, the host reader's side list goes
             through the int64 fix-up

plus the profiling-ring entries each of the large-file cells takes, and the scaled RGB call (which shares the RGB tail)."""
import os
import sys

import numpy as np
import pytest

from conftest import golden_bytes
from helpers import jpeg_optimised_tables
from oracle import orc
from test_gpu_profiling_ring import taken

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rgb_reference as rgb_ref  # noqa: E402
import scaled_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

GPU_READER_FROM = 128 * 1024   # bytes: files of this size and more go to the GPU reader (hvc_capi_jpeg.hip)
ENTRIES = ("planes", "yuv444", "rgb")
PATHS = ("small", "speculated", "refused", "wide_dc")


@pytest.fixture(scope="module")
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


def noise_file(w, h):
    """a 4:2:0 noise frame at quality 90 (the checker's encoder): about 1.2 bytes a pixel"""
    rng = np.random.Generator(np.random.PCG64(5))
    y, u, v = (rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    return orc.encode_yuv(y, u, v, w, h, 420, 90)


def truncated(jpg):
    """cut inside the entropy-coded segment, EOI behind it: the model reads zero bits past the end"""
    import video_coding_amd as hvc
    cut = hvc.hvc.jpeg_read_header(jpg).ecs_offset + 140000
    assert cut < len(jpg) - 50000
    return jpg[:cut] + b"\xff\xd9"


def wide_dc_file(w, h, q=60):
    """DC walks of +-2047 steps far beyond int16 in every component (tests/test_gpu_jpeg_api.py
    test_dc_beyond_int16_decodes_like_the_model), all 63 ACs of every block busy so that the file is a large one"""
    import video_coding_amd as hvc
    qt = np.stack([orc.quant_scale(orc.quant_luma(), q), orc.quant_scale(orc.quant_chroma(), q)])
    info = hvc.hvc.jpeg_encoder_layout(w, h, 420, q)
    rng = np.random.Generator(np.random.PCG64(w + h))
    rec = np.zeros(info.coef_count, dtype=np.int64).reshape(-1, 64)
    rec[:, 1:] = rng.integers(-100, 101, size=(rec.shape[0], 63))
    for i in range(3):
        L = info.layout[i]
        nb = L.blocks_w * L.blocks_h
        steps = rng.choice([-2047, 2047, 2047, 900, 0], size=nb)
        if i == 1:
            steps = -np.abs(steps)
        rec[L.coef_offset // 64:L.coef_offset // 64 + nb, 0] = np.cumsum(steps)
    return jpeg_optimised_tables(w, h, 420, qt, rec.reshape(-1))


class Files:
    """the table's files and, computed once each, what the checker makes of them"""

    def __init__(self):
        odd, even = noise_file(515, 389), noise_file(516, 390)   # odd: the crop and the ceil chroma window; 4:4:4 output: even
        wide = wide_dc_file(368, 272)
        mini = golden_bytes("mini.jpg")
        self.by_path = {"small": (mini, mini), "speculated": (odd, even), "refused": (truncated(odd), truncated(even)),
                        "wide_dc": (wide, wide)}
        self._want = {}

    def file(self, path, entry):
        return self.by_path[path][1 if entry == "yuv444" else 0]

    def want(self, path, entry):
        key = (path, entry)
        if key not in self._want:
            d = orc.Decoder(self.file(path, entry))
            d.decode()
            if entry == "planes":
                self._want[key] = [d.plane(i) for i in range(d.ncomp)]
            elif entry == "yuv444":
                y, u, v = d.get_yuv_frame()
                self._want[key] = np.stack([y, orc.supersample_hv2(u), orc.supersample_hv2(v)])
            else:
                self._want[key] = rgb_ref.planes_to_rgb(d.plane(0), d.plane(1), d.plane(2), 420, d.width, d.height, "interleaved")
        return self._want[key]


@pytest.fixture(scope="module")
def files():
    return Files()


def decode(ctx, entry, jpg):
    """the entry point's output in the form Files.want gives"""
    if entry == "planes":
        info, pixels = ctx.jpeg_decode(jpg)
        return info.planes(pixels)
    if entry == "yuv444":
        return ctx.jpeg_decode_yuv444(jpg)[1]
    return ctx.jpeg_decode_rgb(jpg)[1]


def same(got, want):
    if isinstance(want, list):
        return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    return np.array_equal(got, want)


def test_the_files_are_what_the_paths_need(files):
    for path in PATHS[1:]:
        for jpg in files.by_path[path]:
            assert GPU_READER_FROM <= len(jpg) <= 2 * GPU_READER_FROM, (path, len(jpg))
    for intact, cut in zip(files.by_path["speculated"], files.by_path["refused"]):
        assert cut[:-2] == intact[:len(cut) - 2] and len(cut) < len(intact)
    wide = files.by_path["wide_dc"][0]
    assert np.abs(orc.Decoder(wide).coef_record()).max() > 40000
    assert len(files.by_path["small"][0]) < GPU_READER_FROM


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_point_by_path(ctx, files, entry, path):
    assert same(decode(ctx, entry, files.file(path, entry)), files.want(path, entry))
    if path == "refused":
        # the intact file straight afterwards, on the same context: the fix-up counters and the DC scratch were left consistent
        assert same(decode(ctx, entry, files.file("speculated", entry)), files.want("speculated", entry))


# Ring entries of one call with profiling on.  These figures were taken from the parent commit of the change that put the
# three entry points on one skeleton (as tests/test_gpu_profiling_ring.py does for the small-file cases): the speculated
# block stage is a device-memory call with the context's setting, whatever becomes of the reader's verdict; the host reader's
# second run of the block stage takes none.
RING = {("planes", "speculated"): 1, ("yuv444", "speculated"): 1, ("rgb", "speculated"): 1,
        ("planes", "refused"): 1, ("yuv444", "refused"): 1, ("rgb", "refused"): 1,
        ("planes", "wide_dc"): 1, ("yuv444", "wide_dc"): 1, ("rgb", "wide_dc"): 1}


@pytest.mark.parametrize("path", PATHS[1:])
@pytest.mark.parametrize("entry", ENTRIES)
def test_profiling_ring_entries(ctx, files, entry, path):
    jpg = files.file(path, entry)
    ctx.set_profiling(True)
    try:
        assert taken(ctx) == 0
        got = decode(ctx, entry, jpg)
        ctx.synchronize()
        print("%s %s: %d entries" % (entry, path, taken(ctx)))
        assert taken(ctx) == RING[(entry, path)]
        assert same(got, files.want(path, entry))   # (profiling changes no result)
    finally:
        ctx.set_profiling(False)


def test_scaled_rgb_shares_the_rgb_tail(ctx, files):
    """hvc_jpeg_decode_scaled_rgb at 1/2 on the large odd-sized file: the scaled definition (tools/scaled_reference.py) over
    the checker's record, then the colour definition over those planes"""
    jpg = files.file("speculated", "rgb")
    d = orc.Decoder(jpg)
    rec = d.coef_record()
    n, planes, at = sr.side(2), [], 0
    for i in range(3):
        inf = d.info(i)
        bw, bh = inf["decoded_width"] // 8, inf["decoded_height"] // 8
        planes.append(sr.scaled_plane(rec[at:at + bw * bh * 64], d.array(i, "quant_table"), bw, bh, n))
        at += bw * bh * 64
    w, h = sr.scaled_size(d.width, n), sr.scaled_size(d.height, n)
    assert (w, h) == (258, 195)
    info, got = ctx.jpeg_decode_scaled_rgb(jpg, 2)
    assert (info.width, info.height) == (w, h)
    assert np.array_equal(got, rgb_ref.planes_to_rgb(planes[0], planes[1], planes[2], 420, w, h, "interleaved"))
