"""Every kernel family that takes its (frame, tile) from xcd_work (csrc/hvc_kernels.h), on a grid whose first whole group of
workgroups runs permuted and whose rest runs as dispatched -- what every production-size batch does and the small parity
tests of the families never do (below one group of 8 x 16 workgroups nothing is permuted).  The geometries come from
tests/xcd_grids.py, where tests/test_xcd_grids.py holds them to that condition on the CPU.

Every comparison is exact equality of the WHOLE output buffer over a sentinel fill, against the independent reference the
family's own test module uses (the oracle, the numpy restatements of the RTL twins, tools/libjpeg_reference.py,
tools/scaled_reference.py), never against another GPU call.  Inputs and outputs are device memory, so one call is one
launch.  A tile written for the wrong frame or plane lands in another frame's content, in sentinel bytes, or leaves its own
place at the sentinel."""
import os
import sys

import numpy as np
import pytest

import libjpeg_files as lf
import test_gpu_libjpeg as tl
import test_gpu_mixed as tm
import test_gpu_mixed_encode as te
import test_gpu_mixed_libjpeg as tml
import test_gpu_mixed_scaled as tms
import test_gpu_scaled as ts
import xcd_grids as xg
from helpers import synth_coefs
from oracle import orc
from test_gpu_hardcaml_encoder import blocks_of
from test_gpu_hdec import make_jpeg
from test_guard_bounds import idct_spec, model_pass
from test_hardcaml_encoder_twin import hardcaml_encode_blocks
from test_hardcaml_twin import hardcaml_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import libjpeg_reference as lj  # noqa: E402
import scaled_reference as sr  # noqa: E402
from jpeg_opt_writer import jpeg_optimised_tables  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL16 = 0x5A5A
PLANES, N_FRAMES = xg.TILE_PLANES, xg.TILE_FRAMES
BLOCKS = sum(bw * bh for bw, bh, _ in PLANES)            # per frame: 528 + 72 + 72
EVERY = 50                                                # one block in 50 is made special, over all frames and planes


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd
    return video_coding_amd


@pytest.fixture()
def ctx(hvc):
    c = hvc.Context(0)
    yield c
    c.close()


def table(chroma, quality):
    return orc.quant_scale(orc.quant_chroma() if chroma else orc.quant_luma(), quality).astype(np.uint16)


def special_blocks():
    """(frame, block of the frame's tight record) of every EVERY-th block of the batch: every frame and every plane has some"""
    ids = np.arange(7, N_FRAMES * BLOCKS, EVERY)
    f, b = ids // BLOCKS, ids % BLOCKS
    assert set(f) == set(range(N_FRAMES))
    bounds = np.cumsum([0] + [bw * bh for bw, bh, _ in PLANES])
    assert all(np.count_nonzero((b >= lo) & (b < hi)) > 20 for lo, hi in zip(bounds[:-1], bounds[1:]))
    return f, b


def table_of_block(b):
    bounds = np.cumsum([bw * bh for bw, bh, _ in PLANES])
    return np.array([PLANES[int(np.searchsorted(bounds, x, side="right"))][2] for x in b])


def to_device(*arrays):
    import torch
    out = [torch.from_numpy(np.array(a)).cuda() for a in arrays]   # (a copy: the shared records are read-only)
    torch.cuda.synchronize()          # (torch's copies run on its stream, the launch on the context's)
    return out


def outside_the_model_guard(blocks, q):
    """[n][64] zig-zag records under the table q -> bool [n]: the block leaves the int32 kernel by the guard of
    csrc/hvc_idct_spec.h, restated on the model's passes (test_guard_bounds.model_pass, vectorised over the blocks): the
    coefficient energy, the row-output energy, the arguments of the 181-products of the row and of the column pass (as
    tests/test_gpu_decode.py::test_a_million_blocks_within_one_per_cent_of_each_guard_limit states them)"""
    c = idct_spec()[0]
    b = np.asarray(blocks, dtype=np.int64).reshape(-1, 64)
    d = np.zeros_like(b)
    d[:, np.asarray(orc.zigzag_inverse())] = b * np.asarray(q, dtype=np.int64)
    d = d.reshape(-1, 8, 8)

    def ys(v, col):
        r, s = (4, 3) if col else (0, 0)
        x4, x5, x6, x7 = v[1], v[7], v[5], v[3]
        t = 565 * (x4 + x5) + r
        x4, x5 = (t + (2841 - 565) * x4) >> s, (t - (2841 + 565) * x5) >> s
        t = 2408 * (x6 + x7) + r
        x6, x7 = (t - (2408 - 1609) * x6) >> s, (t - (2408 + 1609) * x7) >> s
        a, b2 = x4 - x6, x5 - x7
        return np.maximum(np.abs(a + b2), np.abs(a - b2))
    row_in = [d[:, :, i] for i in range(8)]                    # element i of every row: [n][8 rows]
    rows = np.stack(model_pass(row_in, False), axis=-1)        # [n][row][column]
    col_in = [rows[:, i, :] for i in range(8)]                 # element i of every column: [n][8 columns]
    energy, renergy = (b * b).sum(axis=1), (rows * rows).sum(axis=(1, 2))
    return (energy > (c["HVC_GUARD_D_PACKED"] // int(np.max(q))) ** 2) | (renergy >= c["HVC_GUARD_RE"]) | \
        (ys(row_in, False).max(axis=1) > c["HVC_GUARD_Y"]) | (ys(col_in, True).max(axis=1) > c["HVC_GUARD_Y"])


def model_wide_blocks(coefs, q, specs):
    """the blocks of a batch [frames][elements] outside the int32 guard"""
    return sum(int(np.count_nonzero(outside_the_model_guard(
        coefs[:, s["coef_offset"]:s["coef_offset"] + s["blocks_w"] * s["blocks_h"] * 64], q[s["qtab"]]))) for s in specs)


# ---- the tile kernels at full size: hvc_decode_frames ---------------------------------------------------------------------
_MODEL = {}


def model_records():
    """(tables, encoder-producible records [frames][elements], the same with every EVERY-th block dense +-2047, the number of
    those blocks): made once, never written again"""
    if not _MODEL:
        q = np.stack([table(0, 75), table(1, 40)])
        rec = np.concatenate([np.concatenate([synth_coefs(5000 + 10 * f + i, bh, bw, q[t])[0].reshape(-1)
                                              for i, (bw, bh, t) in enumerate(PLANES)])[None] for f in range(N_FRAMES)])
        rng = np.random.default_rng(77)
        f, b = special_blocks()
        adv = rec.copy().reshape(N_FRAMES, BLOCKS, 64)
        adv[f, b] = rng.choice(np.array([-2047, 2047], dtype=np.int16), size=(f.size, 64))
        # outside the guard for certain: the coefficient energy alone is beyond (HVC_GUARD_D_PACKED / qmax)^2
        limit = min((idct_spec()[0]["HVC_GUARD_D_PACKED"] // int(t.max())) ** 2 for t in q)
        assert 64 * 2047 ** 2 > limit
        adv = adv.reshape(N_FRAMES, -1)
        for a in (q, rec, adv):
            a.setflags(write=False)
        _MODEL["all"] = (q, rec, adv, int(f.size))
    return _MODEL["all"]


def model_want(coefs, q, specs, fs):
    out = np.full((coefs.shape[0], fs), FILL, dtype=np.uint8)
    for f in range(coefs.shape[0]):
        for s in specs:
            bw, bh = s["blocks_w"], s["blocks_h"]
            blk = coefs[f, s["coef_offset"]:s["coef_offset"] + bw * bh * 64]
            rows = np.arange(bh * 8)[:, None] * s["stride"] + s["plane_offset"] + np.arange(bw * 8)[None, :]
            out[f][rows] = orc.dequant_idct_recon(np.ascontiguousarray(blk), q[s["qtab"]], bw, bh).reshape(bh * 8, bw * 8)
    return out


def decode_frames(hvc, ctx, coefs, q, specs, fs):
    d_c, d_o = to_device(coefs, np.full((coefs.shape[0], fs), FILL, dtype=np.uint8))
    ctx.decode_frames(d_c, coefs.shape[1], q, specs, coefs.shape[0], d_o, fs)
    ctx.synchronize()
    return d_o.cpu().numpy(), ctx.last_wide_blocks()


def test_decode_frames_model(hvc, ctx):
    """k_decode_packed<false>: encoder-producible records, planes spread with gaps and a stride beyond the row"""
    q, rec, _, _ = model_records()
    specs, fs = tl.place(PLANES, "spread")
    assert xg.split(xg.tiles_per_frame(xg.TILE_PLANES), xg.TILE_FRAMES)["full"] == 128
    got, wide = decode_frames(hvc, ctx, rec, q, specs, fs)
    assert np.array_equal(got, model_want(rec, q, specs, fs))
    assert wide == model_wide_blocks(rec, q, specs) == 0


def test_decode_frames_model_blocks_outside_the_guard(hvc, ctx):
    """the fix-up ids are made by permuted workgroups and resolved by k_decode_wide: one block in 50 outside the int32 guard"""
    q, _, adv, n_adv = model_records()
    specs, fs = tl.place(PLANES, "spread")
    got, wide = decode_frames(hvc, ctx, adv, q, specs, fs)
    assert np.array_equal(got, model_want(adv, q, specs, fs))
    assert wide == model_wide_blocks(adv, q, specs) == n_adv


def test_decode_frames_every_block_wide(hvc, ctx):
    """hvc_set_decode_kernel(ctx, 2): k_decode_wide_all on the same grid"""
    q, _, adv, _ = model_records()
    specs, fs = tl.place(PLANES, "spread")
    ctx.set_decode_kernel(2)
    got, wide = decode_frames(hvc, ctx, adv, q, specs, fs)
    assert np.array_equal(got, model_want(adv, q, specs, fs))
    assert wide == N_FRAMES * BLOCKS


def test_decode_frames_hardcaml(hvc, ctx):
    """k_hardcaml: full-range and small records against the numpy restatement of the RTL"""
    rng = np.random.default_rng(31)
    q = np.stack([rng.integers(0, 256, 64), table(1, 75)]).astype(np.uint16)
    coefs = rng.integers(-32768, 32768, (N_FRAMES, BLOCKS, 64)).astype(np.int16)
    coefs[:, ::3] = (coefs[:, ::3] % 64) - 32
    coefs = coefs.reshape(N_FRAMES, -1)
    specs, fs = tl.place(PLANES, "spread")
    want = np.full((N_FRAMES, fs), FILL, dtype=np.uint8)
    for s in specs:
        bw, bh = s["blocks_w"], s["blocks_h"]
        blk = coefs[:, s["coef_offset"]:s["coef_offset"] + bw * bh * 64].reshape(-1, 64)
        px = hardcaml_blocks(blk, q[s["qtab"]]).reshape(N_FRAMES, bh, bw, 8, 8).transpose(0, 1, 3, 2, 4).reshape(N_FRAMES, bh * 8, bw * 8)
        rows = np.arange(bh * 8)[:, None] * s["stride"] + s["plane_offset"] + np.arange(bw * 8)[None, :]
        want[:, rows] = px
    ctx.set_arithmetic("hardcaml")
    got, _ = decode_frames(hvc, ctx, coefs, q, specs, fs)
    assert np.array_equal(got, want)


def test_decode_frames_libjpeg(hvc, ctx):
    """k_islow<false>: ordinary records with lone coefficients exactly at HVC_IS_GUARD_SUM and one step beyond it, both signs"""
    q, coefs = tl.ordinary_record(41, PLANES, N_FRAMES)
    f, b = special_blocks()
    t = table_of_block(b)
    blk = coefs.reshape(N_FRAMES, BLOCKS, 64)
    k = np.arange(f.size)
    pos = np.where(k % 3 == 0, 0, np.where(k % 3 == 1, 63, lj.ZF[8 * 3 + 3]))
    extra, sign = (k // 3) % 2, np.where((k // 6) % 2, -1, 1)
    blk[f, b] = 0
    blk[f, b, pos] = sign * (tl.GUARD // q[t, pos].astype(np.int64) + extra)
    specs, fs = tl.place(PLANES, "spread")
    want, wide = tl.want_buffer(coefs, q, specs, fs)
    assert 0 < wide < f.size and f.size - wide > 100          # both sides of the guard
    ctx.set_arithmetic("libjpeg")
    got, got_wide = decode_frames(hvc, ctx, coefs, q, specs, fs)
    assert np.array_equal(got, want)
    assert got_wide == wide


@pytest.mark.parametrize("layout", ["aligned", "odd"], ids=["dwords", "bytes"])
@pytest.mark.parametrize("scale", ts.SCALES)
def test_decode_frames_scaled(hvc, ctx, scale, layout):
    """k_decode_scaled<N, false, DW>: both store forms; dense blocks of rising amplitude and lone pairs one step on either side
    of the guard of hvc_scaled_spec.h"""
    n = 8 // scale
    q, coefs = ts.ordinary_record(50 + scale, PLANES, N_FRAMES)
    rng = np.random.default_rng(scale)
    f, b = special_blocks()
    t = table_of_block(b)
    blk = coefs.reshape(N_FRAMES, BLOCKS, 64)
    amp = 15 * 2 ** (np.arange(f.size) % 8)
    blk[f, b] = (rng.integers(-1000, 1001, size=(f.size, 64)) * amp[:, None] // 1000).astype(np.int16)
    if n > 1:
        k = sr.spec_constants()
        wa, limit = k["HVC_S%d_GUARD_WA" % n], k["HVC_S%d_GUARD_LIMIT" % n]
        at = sr.ZF[8 * 1 + 1]
        lone = np.arange(0, f.size, 5)
        blk[f[lone], b[lone]] = 0
        blk[f[lone], b[lone], at] = np.where(lone % 2, -1, 1) * ((limit // wa) // q[t[lone], at].astype(np.int64) + (lone // 10) % 2)
    specs, fs = ts.place(PLANES, n, layout)
    assert (fs % 4 == 0 and all((s["plane_offset"] | s["stride"]) % 4 == 0 for s in specs)) == (layout == "aligned")
    want, wide = ts.want_buffer(coefs, q, specs, fs, n)
    assert n == 1 or (60 < wide < f.size - 60)                 # both branches, in permuted and in dispatched workgroups
    got, got_wide = ts.run(ctx, coefs, q, specs, fs, scale, True)
    assert np.array_equal(got, want)
    assert got_wide == wide


# ---- the tile kernels at full size: hvc_encode_frames ---------------------------------------------------------------------
def encode_case(seed):
    """pixel planes spread (noise between the rows' ends and between the planes), coefficient planes 64 elements apart"""
    rng = np.random.default_rng(seed)
    specs, fs = tl.place(PLANES, "spread")
    co = 0
    for s in specs:
        s["coef_offset"] = co + 64
        co = s["coef_offset"] + s["blocks_w"] * s["blocks_h"] * 64
    cfs = co + 128
    pixels = rng.integers(0, 256, size=(N_FRAMES, fs), dtype=np.uint8)
    smooth = rng.integers(100, 140, size=(N_FRAMES, fs), dtype=np.uint8)
    pixels[::2] = smooth[::2]                                  # smooth content too: small coefficients
    return specs, fs, cfs, pixels


def encode_frames(hvc, ctx, pixels, fs, q, specs, cfs):
    d_p, d_c = to_device(pixels, np.full((pixels.shape[0], cfs), FILL16, dtype=np.int16))
    ctx.encode_frames(d_p, fs, q, specs, pixels.shape[0], d_c, cfs)
    ctx.synchronize()
    return d_c.cpu().numpy()


def test_encode_frames_model(hvc, ctx):
    """k_encode: pixels to records against the oracle, the sentinel between the records"""
    q = np.stack([table(0, 75), table(1, 40)])
    specs, fs, cfs, pixels = encode_case(61)
    want = np.full((N_FRAMES, cfs), FILL16, dtype=np.int16)
    for f in range(N_FRAMES):
        for s in specs:
            bw, bh = s["blocks_w"], s["blocks_h"]
            plane = np.ascontiguousarray(pixels[f, s["plane_offset"]:s["plane_offset"] + s["stride"] * bh * 8])
            want[f, s["coef_offset"]:s["coef_offset"] + bw * bh * 64] = orc.fdct_quant(plane, q[s["qtab"]], bw, bh, stride=s["stride"]).reshape(-1)
    assert np.array_equal(encode_frames(hvc, ctx, pixels, fs, q, specs, cfs), want)


def test_encode_frames_hardcaml(hvc, ctx):
    """k_hardcaml_encode against the numpy restatement of the RTL encoder"""
    q = np.stack([table(0, 95), table(1, 50)])
    specs, fs, cfs, pixels = encode_case(62)
    want = np.full((N_FRAMES, cfs), FILL16, dtype=np.int16)
    for f in range(N_FRAMES):
        for s in specs:
            bw, bh = s["blocks_w"], s["blocks_h"]
            plane = pixels[f, s["plane_offset"]:s["plane_offset"] + s["stride"] * bh * 8].reshape(bh * 8, s["stride"])
            want[f, s["coef_offset"]:s["coef_offset"] + bw * bh * 64] = hardcaml_encode_blocks(blocks_of(plane, bw, bh), q[s["qtab"]]).reshape(-1)
    ctx.set_encode_arithmetic("hardcaml")
    assert np.array_equal(encode_frames(hvc, ctx, pixels, fs, q, specs, cfs), want)


# ---- the mixed kernels: a workgroup is 4 units of 64 blocks of one plane, the grid is one row of groups ---------------------
def table_pair(i):
    return [[table(0, 75), table(1, 75)], [table(0, 40), table(1, 90)], [table(1, 60), table(0, 85)]][i % 3]


_MIXED = {}


def mixed_frames(adversarial):
    """the set of xg.MIXED_ORDER through test_gpu_mixed.make_frame, every frame with a seed of its own, three table pairs in
    turn; adversarial: every EVERY-th block of the set dense +-2047 -> (frames, the number of those blocks)"""
    if adversarial not in _MIXED:
        rng = np.random.default_rng(88)
        frames, n_adv, at = [], 0, 3
        for i, planes in enumerate(xg.mixed_set(xg.MIXED_ORDER)):
            tables, coefs = table_pair(i), None
            if adversarial:
                coefs = []
                for k, (bw, bh, t) in enumerate(planes):
                    if not bw * bh:
                        coefs.append(None)
                        continue
                    c = synth_coefs(7000 + 10 * i + k, bh, bw, tables[t])[0].copy().reshape(-1, 64)
                    hit = np.arange(at % EVERY, bw * bh, EVERY)
                    c[hit] = rng.choice(np.array([-2047, 2047], dtype=np.int16), size=(hit.size, 64))
                    at += EVERY - (bw * bh) % EVERY              # (keeps the stride of EVERY across planes, roughly)
                    n_adv += hit.size
                    coefs.append(c.reshape(bh, bw, 64))
            frames.append(tm.make_frame(planes, tables, 7000 + 10 * i, coefs=coefs))
        _MIXED[adversarial] = (frames, n_adv)
    return _MIXED[adversarial]


def mixed_wide_blocks(frames):
    n = 0
    for fr in frames:
        at = 0
        for bw, bh, t in fr["planes"]:
            n += int(np.count_nonzero(outside_the_model_guard(fr["coefs"][at:at + bw * bh * 64], fr["tables"][t]))) if bw * bh else 0
            at += bw * bh * 64
    return n


def mixed_want(frames, po, size, fill=0x5A):
    out = np.full(size, fill, dtype=np.uint8)
    for fr, off in zip(frames, po):
        out[off:off + fr["want"].size] = fr["want"]
    return out


def test_decode_frames_mixed(hvc, ctx):
    """k_decode_mixed: `group = wf * gridDim.x + wt` under the permutation, the last group with spare units"""
    frames, _ = mixed_frames(False)
    assert xg.mixed_units([fr["planes"] for fr in frames]) % xg.MIXED_GROUP != 0
    got, po = tm.run_mixed(ctx, frames, True)
    assert np.array_equal(got, mixed_want(frames, po, got.size))
    assert ctx.last_wide_blocks() == mixed_wide_blocks(frames) == 0


def test_decode_frames_mixed_blocks_outside_the_guard(hvc, ctx):
    """k_decode_mixed_wide resolves the ids (unit * 64 + lane) that permuted groups wrote"""
    frames, n_adv = mixed_frames(True)
    assert n_adv > 600
    got, po = tm.run_mixed(ctx, frames, True)
    assert np.array_equal(got, mixed_want(frames, po, got.size))
    assert ctx.last_wide_blocks() == mixed_wide_blocks(frames) == n_adv


@pytest.mark.parametrize("placement", ["dwords", "bytes"])
@pytest.mark.parametrize("scale", tms.SCALES)
def test_decode_frames_mixed_scaled(hvc, ctx, scale, placement):
    """k_decode_mixed_scaled<N>: both store forms; at 1/2 some of the module's ordinary blocks leave the int32 guard under the
    coarser table pairs, so both branches run there"""
    n = 8 // scale
    frames = [tms.frame_of(hvc, planes, table_pair(i), 300 + 10 * i) for i, planes in enumerate(xg.mixed_set(xg.MIXED_ORDER))]
    infos, po, size = tms.place(hvc, frames, n, placement)
    want, wide = tms.want_buffer(frames, infos, po, size, n)
    got = tms.run_frames(ctx, frames, infos, po, size, scale, True)
    assert np.array_equal(got, want)
    assert ctx.last_wide_blocks() == wide and (wide > 0) == (n == 4)


def test_encode_frames_mixed(hvc, ctx):
    """k_encode_mixed: pixel records to coefficient records, the sentinel between the records"""
    frames = [te.make_frame(planes, table_pair(i), 400 + 10 * i) for i, planes in enumerate(xg.mixed_set(xg.MIXED_ORDER_NO_ZERO))]
    co, _, _, want = te.place(frames)
    for fr, off in zip(frames, co):
        want[off:off + fr["want"].size] = fr["want"]
    got, got_co = te.run_mixed(ctx, frames, True)
    assert got_co == co and np.array_equal(got, want)


def test_decode_frames_mixed_libjpeg(hvc, ctx):
    """k_islow_mixed: lone coefficients exactly at HVC_IS_GUARD_SUM and one step beyond it in every plane"""
    frames, at = [], 3
    for i, planes in enumerate(xg.mixed_set(xg.MIXED_ORDER_NO_ZERO)):
        fr = tml.frame(planes, tml.ordinary_tables(20 + i % 3), 500 + 10 * i)
        blk, first = fr["coefs"].reshape(-1, 64), 0
        for bw, bh, t in planes:
            hit = first + np.arange(at % EVERY, bw * bh, EVERY)
            at += EVERY - (bw * bh) % EVERY
            first += bw * bh
            k = np.arange(hit.size)
            pos = np.where(k % 2, 63, 0)
            blk[hit] = 0
            blk[hit, pos] = np.where((k // 2) % 2, -1, 1) * (tl.GUARD // fr["tables"][t][pos].astype(np.int64) + (k // 4 + i) % 2)
        frames.append(fr)
    want, wide = tml.want_planes(frames, "spread")
    assert wide > 100
    ctx.set_mixed_arithmetic("libjpeg")
    got, got_wide = tml.run_planes(ctx, frames, True, "spread")
    assert np.array_equal(got, want)
    assert got_wide == wide


# ---- the DCP instantiations: the compact DC array of the GPU Huffman reader, indexed by the permuted frame --------------------
_FILES = {}


def reader_files(hvc):
    """xg.READER_FILES baseline files of xg.READER_SIZE 4:2:0 with one set of quantiser tables (a uniform batch's rule):
    the even ones as the oracle's encoder writes them at quality 75; the odd ones carry a quality-90 encoding's record (larger
    coefficients) under the same tables, with Huffman tables fitted to the file"""
    if not _FILES:
        w, h = xg.READER_SIZE
        files = []
        for f in range(xg.READER_FILES):
            if f % 2 == 0:
                files.append(make_jpeg(3000 + 5 * f, w, h, 420, 75))
            else:
                _, rec = hvc.hvc.jpeg_entropy_decode(make_jpeg(3000 + 5 * f, w, h, 420, 90))
                q = hvc.hvc.jpeg_read_header(files[0]).qtab_array()
                files.append(jpeg_optimised_tables(w, h, 420, q, rec))
        info = hvc.hvc.jpeg_read_header(files[0])
        assert [(info.layout[k].blocks_w, info.layout[k].blocks_h, info.layout[k].qtab) for k in range(3)] == xg.READER_PLANES
        _FILES["all"] = files
    return _FILES["all"]


def reader_batch(ctx, jpegs, fs, scale=None):
    """one chunk of all the files through the GPU reader into device memory over FILL -> the buffer [files][fs]"""
    import torch
    out = torch.full((len(jpegs), fs), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if scale is None:
        st = ctx.jpeg_decode_batch(jpegs, out, fs, threads=2, frames_per_chunk=len(jpegs), gpu_entropy=True)
    else:
        st = ctx.jpeg_decode_batch_scaled(jpegs, scale, out, fs, threads=2, frames_per_chunk=len(jpegs), gpu_entropy=True)
    ctx.synchronize()
    # one chunk = one launch of 64 frames, and the GPU reader took it: the host reader, which leaves no DC array, reports its time
    assert st.chunks == 1 and st.frames_per_chunk == xg.READER_FILES and st.entropy_ms_sum == 0
    return out.cpu().numpy()


def test_gpu_reader_batch_model(hvc, ctx):
    """k_decode_packed<true> against the oracle decoder.  The odd files' records are no encoder's at their tables: most of
    their noisy blocks leave the int32 kernel by the row-output energy, so k_decode_wide resolves ids made under the
    permutation here as well, with the DC of the compact array"""
    jpegs = reader_files(hvc)
    info = hvc.hvc.jpeg_read_header(jpegs[0])
    fs = info.pixel_bytes + 24
    want = np.full((len(jpegs), fs), FILL, dtype=np.uint8)
    wide = 0
    for f, j in enumerate(jpegs):
        d = orc.Decoder(j)
        d.decode()
        want[f, :info.pixel_bytes] = tl.padded_record(info, [d.plane(k) for k in range(3)])
        _, rec = hvc.hvc.jpeg_entropy_decode(j)
        q = info.qtab_array()
        wide += sum(int(np.count_nonzero(outside_the_model_guard(rec[L.coef_offset:L.coef_offset + L.blocks_w * L.blocks_h * 64], q[L.qtab])))
                    for L in info.layout[:3])
    assert np.array_equal(reader_batch(ctx, jpegs, fs), want)
    assert ctx.last_wide_blocks() == wide > 1000


def test_gpu_reader_batch_libjpeg(hvc, ctx):
    """k_islow<true> against tools/libjpeg_reference.py"""
    jpegs = reader_files(hvc)
    info = hvc.hvc.jpeg_read_header(jpegs[0])
    fs = info.pixel_bytes + 24
    want = np.full((len(jpegs), fs), FILL, dtype=np.uint8)
    for f, j in enumerate(jpegs):
        fi, coefs = tl.file_record(hvc, j)
        want[f, :info.pixel_bytes] = tl.padded_record(info, lj.record_planes(coefs, fi.qtab_array(), lf.planes_of_info(fi)))
    ctx.set_arithmetic("libjpeg")
    assert np.array_equal(reader_batch(ctx, jpegs, fs), want)


@pytest.mark.parametrize("scale", [2, 8])
def test_gpu_reader_batch_scaled(hvc, ctx, scale):
    """k_decode_scaled<N, true, DW> against tools/scaled_reference.py; at 1/8 the decode reads the DC array alone"""
    jpegs = reader_files(hvc)
    rows = [np.concatenate([p.reshape(-1) for p in ts.definition_of_file(hvc, j, scale)[1]]) for j in jpegs]
    fs = rows[0].size + 3
    want = np.full((len(jpegs), fs), FILL, dtype=np.uint8)
    want[:, :-3] = np.stack(rows)
    assert np.array_equal(reader_batch(ctx, jpegs, fs, scale), want)
