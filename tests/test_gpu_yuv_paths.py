"""Every vector and scalar path of the `oyuv convert` kernels (csrc/hvc_yuv.hip, and K2 of csrc/hvc_kernels.hip).

Each kernel has a packed-byte vector body and a per-sample scalar body.  The launchers choose once per launch, from the
alignment of the bases, the row strides and the plane strides; the kernel chooses again per lane, from whether the lane's group
of samples is whole.  The tables below are built so that every (kernel, choice) cell runs: the vector form on rows with a
ragged last group, the scalar form for each single reason the launcher can have, the fused chroma kernels' and the packing
kernels' scalar bodies, misaligned device bases, the crop kernel's unaligned loads and clamps, and the XCD workgroup
permutation through the plane-operation entry points.

Expected bytes come from the restated tools (oracle/) alone.  Every output buffer is pre-filled with a constant and compared
whole: the padding between rows, planes and frames and the guard bytes around the region must keep their fill, also where the
kernels write the caller's device memory directly.  The selection predicates restated here are bookkeeping: they say which
cell a case landed in, so that a table that loses a cell fails (the census), and nothing else."""
import collections
import itertools

import numpy as np
import pytest

from oracle import orc

FILL = 0xA5
GUARD = 48                # bytes in front of and behind every region
ARENA = 4 << 20           # device bytes for sources and for destinations; the largest case (B4) is 1.4 MB
PACKED = ("YUY2", "UYVY", "YVYU")
FORMATS = [420, 422, 444, "YUY2", "UYVY", "YVYU"]


def pad16(n):
    """the next multiple of 16 above n: an aligned stride that always leaves padding behind the row"""
    return (n + 16) // 16 * 16


# ---- the launchers' selection predicates, restated (coverage bookkeeping only) --------------------------------------------------
# bytes a lane loads / stores at once in the vector form (launch_plane_op's sa, da); k_crop's loads take any alignment
LANE_BYTES = {"k_subsample420": (16, 8), "k_subsample422": (16, 8), "k_upsample422": (8, 16), "k_crop": (1, 8),
              "k_chroma_420_to_422": (8, 8), "k_chroma_422_to_420": (8, 8)}
BY_SOURCE = ("k_upsample422", "k_chroma_420_to_422")       # a lane = 8 source samples; else 8 destination samples

Launch = collections.namedtuple("Launch", "kernel sw sh dw dh src src_stride src_ps dst dst_stride dst_ps")


def failed_terms(src, src_stride, src_ps, sa, dst, dst_stride, dst_ps, da):
    t = set()
    for what, value, a in (("src base", src, sa), ("src stride", src_stride, sa), ("src plane stride", src_ps, sa),
                           ("dst base", dst, da), ("dst stride", dst_stride, da), ("dst plane stride", dst_ps, da)):
        if value % a:
            t.add(what)
    return t


def scalar_reason(t):
    """one name for why the launcher left the vector form: a base alone, else the row strides (the plane strides of tight
    planes follow from them), else the plane strides alone"""
    if t == {"src base"} or t == {"dst base"}:
        return "scalar by %s" % min(t)
    if t & {"src base", "dst base"}:
        return "scalar by a base and more"
    if t & {"src stride", "dst stride"}:
        return "scalar by row stride"
    return "scalar by plane stride"


def plane_op_cells(L):
    """launch_plane_op's P.vec and the kernels' per-lane `8 g + 8 <= width` -> the cells the launch lands in"""
    sa, da = LANE_BYTES[L.kernel]
    t = failed_terms(L.src, L.src_stride, L.src_ps, sa, L.dst, L.dst_stride, L.dst_ps, da)
    if t:
        return [scalar_reason(t)]
    gw = L.sw if L.kernel in BY_SOURCE else L.dw
    cells = ["vec, whole" if gw % 8 == 0 else "vec, less than one group" if gw < 8 else "vec, ragged"]
    if L.src % 16 == 8 or L.dst % 16 == 8:
        cells.append("vec, a base at 8 mod 16")
    return cells


def crop_cells(L, x, y):
    """k_crop's own branches on top: the 8-byte load from any alignment, and the clamped columns / rows"""
    cells = plane_op_cells(L)
    if not cells[0].startswith("vec"):
        return cells
    for g in range(L.dw // 8):
        if 8 * g + x >= 0 and 8 * g + x + 8 <= L.sw:
            cells.append("vec, load at %d mod 8" % ((L.src + 8 * g + x) % 8))
            break
    for name, out in (("left", x < 0), ("right", x + L.dw > L.sw), ("top", y < 0), ("bottom", y + L.dh > L.sh)):
        if out:
            cells.append("vec, clamped %s" % name)
    return cells


def k2_cells(L):
    """launch_upsample420's x8 / vec / scalar split"""
    cw = L.sw
    t8 = failed_terms(L.src, L.src_stride, L.src_ps, 8, L.dst, L.dst_stride, L.dst_ps, 16)
    t4 = failed_terms(L.src, L.src_stride, L.src_ps, 4, L.dst, L.dst_stride, L.dst_ps, 8)
    if cw % 8 == 0 and not t8:
        return ["x8"]
    if cw % 4 == 0 and not t4:
        return ["vec4 by width"] if cw % 8 else [scalar_reason(t8).replace("scalar", "vec4")]
    return ["scalar by width"] if cw % 4 else [scalar_reason(t4)]


def packed_cells(w, pk, py, pu, pv, packed_fs, planar_fs, luma_fs):
    """launch_packed_op's P.vec (a vector lane is whole by construction: w % 8 == 0)"""
    if w % 8:
        return ["scalar by width"]
    t = set()
    for what, value, a in (("packed base", pk, 16), ("luma base", py, 8), ("chroma base", pu, 4), ("chroma base", pv, 4),
                           ("frame stride", packed_fs, 16), ("frame stride", planar_fs, 4), ("frame stride", luma_fs, 8)):
        if value % a:
            t.add(what)
    return ["vec"] if not t else ["scalar by %s" % min(t)] if len(t) == 1 else ["scalar by several terms"]


def chroma_size(fmt, w, h):
    return (w if fmt == 444 else w // 2), (h // 2 if fmt == 420 else h)


def frame_bytes(fmt, w, h):
    if fmt in PACKED:
        return 2 * w * h
    cw, ch = chroma_size(fmt, w, h)
    return w * h + 2 * cw * ch


SCRATCH_A, SCRATCH_B = 1 << 30, 1 << 31      # hvc_yuv_convert's two scratch arrays: device allocations of their own, aligned


def convert_launches(fi, fo, size_in, size_out, off, S, D):
    """hvc_yuv_convert's routing: which kernels a call launches, on which addresses and strides -> (routes, [(kernel, cells)])"""
    (w, h), (w2, h2), (xo, yo) = size_in, size_out, off
    A, B = SCRATCH_A, SCRATCH_B
    packed_in, packed_out = fi in PACKED, fo in PACKED
    in_planar, out_planar = (422 if packed_in else fi), (422 if packed_out else fo)
    sp, dp = w * h, w2 * h2
    in_fs, out_fs, a_fs, b_fs = frame_bytes(fi, w, h), frame_bytes(fo, w2, h2), 4 * sp, 5 * dp
    same = (w, h) == (w2, h2) and (xo, yo) == (0, 0)
    dcw, dch = chroma_size(out_planar, w2, h2)
    scw, sch = chroma_size(in_planar, w, h)
    oy, o_fs = (B + 3 * dp, b_fs) if packed_out else (D, out_fs)
    ou, ov = oy + dp, oy + dp + dcw * dch
    direct = same and out_planar == 444 and in_planar != 444
    luma_direct = same and packed_in and not packed_out
    luma_in_place = same and packed_out
    fused = same and {in_planar, out_planar} == {420, 422}
    window = (not same and out_planar != 444 and xo >= 0 and yo >= 0 and xo + w2 <= w and yo + h2 <= h and xo % 16 == 0 and
              w % 16 == 0)
    routes = [name for name, on in (("direct", direct), ("luma_direct", luma_direct), ("luma_in_place", luma_in_place),
                                    ("chroma_fused", fused), ("window", window)) if on]
    if not same and not window and out_planar != 444:
        routes.append("materialised crop")
    out = []
    py, pu, pv, p_fs = S, S + sp, S + sp + scw * sch, in_fs
    if packed_in:
        out.append(("k_unpack422", packed_cells(w, S, oy if luma_direct else A, A + sp, A + sp + sp // 2, in_fs, a_fs,
                                                o_fs if luma_direct else a_fs)))
        py, pu, pv, p_fs = A, A + sp, A + sp + sp // 2, a_fs
    full, full_fs = [pu, pv], [p_fs, p_fs]
    if in_planar != 444 and not fused:
        full, full_fs = ([ou, ov], [o_fs] * 2) if direct else ([A + 2 * sp, A + 3 * sp], [a_fs] * 2)
        for k, c in enumerate((pu, pv)):
            if in_planar == 420:
                out.append(("K2", k2_cells(Launch("K2", w // 2, h // 2, w, h, c, w // 2, p_fs, full[k], w, full_fs[k]))))
            else:
                out.append(("k_upsample422", plane_op_cells(Launch("k_upsample422", w // 2, h, w, h, c, w // 2, p_fs, full[k], w,
                                                                   full_fs[k]))))
    if not same:
        out.append(("k_crop", crop_cells(Launch("k_crop", w, h, w2, h2, py, w, p_fs, oy, w2, o_fs), xo, yo)))
    for k in range(2):
        od = (ou, ov)[k]
        if fused and in_planar == 420:
            out.append(("k_chroma_420_to_422", plane_op_cells(Launch("k_chroma_420_to_422", w // 2, h // 2, w2 // 2, h2, full[k],
                                                                     w // 2, full_fs[k], od, w2 // 2, o_fs))))
        elif fused:
            out.append(("k_chroma_422_to_420", plane_op_cells(Launch("k_chroma_422_to_420", w // 2, h, w2 // 2, h2 // 2, full[k],
                                                                     w // 2, full_fs[k], od, w2 // 2, o_fs))))
        if fused or direct:
            continue
        src, src_fs, stride = full[k], full_fs[k], w2
        if window:
            src, stride = src + yo * w + xo, w
        elif not same:
            src, src_fs = (od, o_fs) if out_planar == 444 else (B + k * dp, b_fs)
            out.append(("k_crop", crop_cells(Launch("k_crop", w, h, w2, h2, full[k], w, full_fs[k], src, w2, src_fs), xo, yo)))
        if out_planar == 420:
            out.append(("k_subsample420", plane_op_cells(Launch("k_subsample420", w2, h2, w2 // 2, h2 // 2, src, stride, src_fs, od,
                                                                w2 // 2, o_fs))))
        elif out_planar == 422:
            out.append(("k_subsample422", plane_op_cells(Launch("k_subsample422", w2, h2, w2 // 2, h2, src, stride, src_fs, od,
                                                                w2 // 2, o_fs))))
    if packed_out:
        out.append(("k_pack422", packed_cells(w2, D, py if luma_in_place else oy, ou, ov, out_fs, b_fs,
                                              p_fs if luma_in_place else b_fs)))
    return routes, out


# ---- B1 / B4: the plane-operation entry points -----------------------------------------------------------------------------------
ENTRY_KERNEL = {"subsample420": "k_subsample420", "subsample422": "k_subsample422", "upsample422": "k_upsample422",
                "crop_planes": "k_crop", "upsample420": "K2"}
PlaneCase = collections.namedtuple("PlaneCase", "entry sw sh dw dh x y n_planes src_stride dst_stride src_ps dst_ps src_off dst_off "
                                                "device")


def make_case(entry, gw, rows, n_planes, device, odd=0, src_off=0, dst_off=0, ss=0, ds=0, sps=0, dps=0, window=None):
    """a case whose lane grid is gw samples x rows: aligned padded strides and plane strides, plus what the arguments add"""
    x = y = 0
    if entry == "subsample420":
        sw, sh, dw, dh = 2 * gw + odd, 2 * rows + odd, gw, rows
    elif entry == "subsample422":
        sw, sh, dw, dh = 2 * gw + odd, rows, gw, rows
    elif entry == "upsample422":
        sw, sh, dw, dh = gw, rows, 2 * gw, rows
    elif entry == "upsample420":
        sw, sh, dw, dh = gw, rows, 2 * gw, 2 * rows
    else:
        (sw, sh, x, y), dw, dh = window or (gw + 5, rows + 2, 2, 1), gw, rows
    src_stride, dst_stride = pad16(sw) + ss, pad16(dw) + ds
    return PlaneCase(entry, sw, sh, dw, dh, x, y, n_planes, src_stride, dst_stride, pad16(src_stride * sh) + 16 + sps,
                     pad16(dst_stride * dh) + 16 + dps, src_off, dst_off, device)


RAGGED = (9, 15, 17)                 # group widths 9, 15 and 8 k + 1 with k >= 2
GRID = list(itertools.product((False, True), (1, 2, 5), (1, 3)))      # memory x rows of lanes x planes


def b1_cases(entry):
    """every selection cell of one entry point, at 1, 2 and 5 rows of lanes, 1 and 3 planes, host and device memory"""
    for device, rows, n_planes in GRID:
        def mk(gw, **kw):
            return make_case(entry, gw, rows, n_planes, device, **kw)
        if entry == "upsample420":
            for cw in (8, 16, 24, 4, 12, 20, 1, 2, 3, 5, 6, 7) + RAGGED:     # x8; one dword per lane; scalar by width
                yield mk(cw)
            for cw in (8, 16):                                               # strides that allow the dword form only
                yield mk(cw, ss=4)
                yield mk(cw, ds=8)
                if n_planes == 3:
                    yield mk(cw, sps=4)
                    yield mk(cw, dps=8)
            for cw in (8, 12, 16):
                yield mk(cw, ss=1)
                yield mk(cw, ds=1)
                if n_planes == 3:
                    yield mk(cw, sps=1)
                    yield mk(cw, dps=1)
                if device:
                    for o in (1, 4, 8):
                        yield mk(cw, src_off=o)
                        yield mk(cw, dst_off=o)
            continue
        for gw in (8, 16, 24) + RAGGED + (25,) + tuple(range(1, 8)):        # vec: whole, ragged, less than one group
            yield mk(gw)
        if entry in ("subsample420", "subsample422"):
            yield mk(17, odd=1)                                              # (the source's last column / row is not used)
        for gw in RAGGED:
            yield mk(gw, ss=1)                                               # scalar by row stride
            yield mk(gw, ds=1)
            if n_planes == 3:                                                # scalar by plane stride: plane 0 alone is aligned
                yield mk(gw, sps=1)
                yield mk(gw, dps=1)
            if device:                                                       # scalar by base; + 4 and + 8 tell 16 from 8 bytes
                for o in (1, 4, 8):
                    yield mk(gw, src_off=o)
                    yield mk(gw, dst_off=o)
        if entry == "crop_planes":
            for dw, x in itertools.product((8, 17), range(10)):              # windows inside: the 8-byte load at any alignment
                yield mk(dw, window=(dw + 12, rows + 2, x, 1))
            for win in ((20, rows + 1, -3, 0), (20, rows + 1, 8, 0), (20, rows + 1, 1, -2), (20, rows + 1, 1, 2),
                        (20, rows + 1, -3, -2), (20, rows + 1, 8, 2)):       # clamped left, right, top, bottom, at two corners
                yield mk(17, window=win)
            yield mk(33, window=(20, max(1, rows - 1), -3, -1))              # larger than the source on every side


def b1_required(entry):
    """the (cell, device, rows, n_planes) that must have run for one entry point"""
    if entry == "upsample420":
        # unreachable: "vec, ragged" -- launch_upsample420 takes a vector form only for a whole number of groups (cw % 4, cw % 8)
        cells = ["x8", "vec4 by width", "vec4 by row stride", "scalar by width", "scalar by row stride"]
        planes3 = ["vec4 by plane stride", "scalar by plane stride"]
        dev = ["vec4 by src base", "vec4 by dst base", "scalar by src base", "scalar by dst base"]
    else:
        cells = ["vec, whole", "vec, ragged", "vec, less than one group", "scalar by row stride"]
        planes3 = ["scalar by plane stride"]
        dev = ["scalar by src base", "scalar by dst base", "vec, a base at 8 mod 16"]
        if entry == "crop_planes":
            # unreachable: "scalar by src base" -- k_crop's predicate does not look at the source: its loads take any alignment
            dev.remove("scalar by src base")
            cells += ["vec, load at %d mod 8" % k for k in range(8)] + ["vec, clamped %s" % e for e in ("left", "right", "top", "bottom")]
    need = set()
    for device, rows, n_planes in GRID:
        for c in cells + (planes3 if n_planes == 3 else []) + (dev if device else []):
            need.add((c, device, rows, n_planes))
    return need


def case_cells(c, src_addr, dst_addr):
    L = Launch(ENTRY_KERNEL[c.entry], c.sw, c.sh, c.dw, c.dh, src_addr, c.src_stride, c.src_ps, dst_addr, c.dst_stride, c.dst_ps)
    return k2_cells(L) if L.kernel == "K2" else crop_cells(L, c.x, c.y) if L.kernel == "k_crop" else plane_op_cells(L)


# B4: 9 planes whose lane grid is 260 (K2's wide form: 264) samples x 131 rows.  ceil(260 / 8) = 33 groups x 131 rows = 4323
# lanes = 17 workgroups of 256 per plane, 9 x 17 = 153 workgroups: xcd_work permutes the first 128 (one whole group of 8 XCDs x
# runs of 16) and leaves 25 as dispatched; 17 is no power of two, so planes begin and end inside the permuted runs.
def b4_case(entry, device):
    if entry == "crop_planes":
        return make_case(entry, 260, 131, 9, device, window=(300, 150, 45, 25))    # (clamps at the right and at the bottom)
    return make_case(entry, 264 if entry == "upsample420" else 260, 131, 9, device)


def b4_workgroups(c):
    gw, rows = (c.sw, c.sh) if c.entry in ("upsample422", "upsample420") else (c.dw, c.dh)
    return -(-(-(-gw // 8) * rows) // 256)


# ---- B2 / B3: hvc_yuv_convert ---------------------------------------------------------------------------------------------------
B2_SIZES = ((2, 2), (6, 2), (8, 2), (16, 2), (18, 6), (36, 10), (70, 34), (72, 6), (80, 4))
B2_BASES = ((False, 0, 0), (True, 0, 0), (True, 1, 0), (True, 0, 1), (True, 4, 0), (True, 0, 4), (True, 4, 4))    # device, src, dst


def b2_required():
    need = set()
    for device in (False, True):
        for k in ("k_chroma_420_to_422", "k_chroma_422_to_420"):
            # unreachable: "vec, ragged" and "vec, less than one group" -- the strides are tight, so the vector form (stride % 8
            # == 0) means whole groups; "scalar by plane stride" -- the frame sizes of such widths are multiples of 8
            need |= {(k, c, device) for c in ("vec, whole", "scalar by row stride")}
            if device:
                need |= {(k, c, device) for c in ("scalar by src base", "scalar by dst base")}
        for k in ("k_unpack422", "k_pack422"):
            # unreachable: "scalar by chroma base", "scalar by frame stride" -- the planar side's chroma planes live in the
            # call's own scratch, and with w % 8 == 0 every frame size is a multiple of 16
            need |= {(k, c, device) for c in ("vec", "scalar by width")}
            if device:
                need |= {(k, c, device) for c in ("scalar by packed base", "scalar by luma base")}
        need |= {("route", r, device) for r in ("direct", "luma_direct", "luma_in_place", "chroma_fused")}
        for k in ("k_upsample422", "k_subsample420", "k_subsample422"):
            need |= {(k, c, device) for c in ("vec, whole", "scalar by row stride")}
        need |= {("K2", c, device) for c in ("x8", "vec4 by width", "scalar by width")}
    return need


# (source size, output size, offset): the window read in place (x_off % 16 == 0, src_w % 16 == 0) with a whole and with a ragged
# sub-sampled row, the materialised crop (a source width or an offset that is no multiple of 16), a negative offset, an output
# larger than the source
B3_GEOMETRIES = (((96, 40), (48, 24), (16, 6)), ((96, 40), (32, 30), (64, 10)), ((96, 40), (52, 24), (16, 6)),
                 ((128, 12), (36, 8), (32, 3)), ((100, 40), (48, 24), (16, 6)), ((70, 34), (32, 16), (9, 5)),
                 ((96, 40), (34, 20), (24, 1)), ((32, 16), (48, 40), (-6, -4)), ((32, 16), (64, 32), (0, 0)),
                 ((32, 16), (128, 18), (-48, -1)))
B3_OUTPUTS = (420, 422, "UYVY")
B3_BASES = ((0, 0), (1, 0), (0, 1), (8, 8))


def b3_class(routes, size_in, size_out, off):
    if "window" in routes:
        return "window, %s sub-sampled row" % ("whole" if size_out[0] // 2 % 8 == 0 else "ragged")
    if off[0] < 0 or off[1] < 0:
        return "materialised, negative offset"
    if size_out[0] > size_in[0] and size_out[1] > size_in[1]:
        return "materialised, larger than the source"
    return "materialised, inside"


B3_CLASSES = ("window, whole sub-sampled row", "window, ragged sub-sampled row", "materialised, inside",
              "materialised, negative offset", "materialised, larger than the source")


# ---- the tables against the census, without a GPU (nominal addresses: aligned arenas) ------------------------------------------
def missing(need, hit):
    return sorted(map(str, need - hit))


@pytest.mark.parametrize("entry", list(ENTRY_KERNEL))
def test_plane_op_table_reaches_every_cell(entry):
    hit = set()
    for c in b1_cases(entry):
        for cell in case_cells(c, c.src_off if c.device else 0, c.dst_off if c.device else 0):
            hit.add((cell, c.device, c.dh if entry != "upsample420" else c.sh, c.n_planes))
    assert not missing(b1_required(entry), hit)
    c = b4_case(entry, True)
    assert b4_workgroups(c) == 17 and c.n_planes * 17 == 153 > 128 and 153 % 128 and case_cells(c, 0, 0)[0] in ("vec, ragged", "x8")


def test_convert_tables_reach_every_cell():
    hit = set()
    for fi, fo, size, (device, so, do) in itertools.product(FORMATS, FORMATS, B2_SIZES, B2_BASES):
        routes, launches = convert_launches(fi, fo, size, size, (0, 0), so, do)
        hit |= {("route", r, device) for r in routes} | {(k, c, device) for k, cells in launches for c in cells}
    assert not missing(b2_required(), hit)
    hit = set()
    for fi, fo, (si, so_, off) in itertools.product(FORMATS, B3_OUTPUTS, B3_GEOMETRIES):
        hit.add((b3_class(convert_launches(fi, fo, si, so_, off, 0, 0)[0], si, so_, off), fo))
    assert not missing(set(itertools.product(B3_CLASSES, B3_OUTPUTS)), hit)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
class Device:
    """two device arenas; a case's region starts where the test puts it, so the base address's alignment is the test's choice"""

    def __init__(self):
        import torch
        self.torch = torch
        self.src = torch.empty(ARENA, dtype=torch.uint8, device="cuda")
        self.dst = torch.empty(ARENA, dtype=torch.uint8, device="cuda")


@pytest.fixture(scope="module")
def gpu():
    import torch
    import video_coding_amd as hvc
    ctx, dev = hvc.Context(0), Device()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)       # (ordered with torch's copies and fills of the arenas)
    yield ctx, dev
    ctx.synchronize()
    ctx.reset_stream()
    ctx.close()


def start_for(base, off):
    """the first index >= GUARD at which base + index = off (mod 16)"""
    return GUARD + (off - base - GUARD) % 16


def run(dev, device, src, s0, want, d0, call):
    """call(source from s0 on, destination from d0 on) on host or device memory -> the whole destination buffer afterwards"""
    assert src.size <= ARENA and want.size <= ARENA
    if not device:
        got = np.full(want.size, FILL, np.uint8)
        call(src[s0:], got[d0:])
        return got
    dev.src[:src.size].copy_(dev.torch.from_numpy(src))
    d = dev.dst[:want.size]
    d.fill_(FILL)
    call(dev.src[s0:], dev.dst[d0:])
    return d.cpu().numpy()          # (the same stream: after the kernels)


def first_difference(got, want, d0):
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else "%d bytes differ, first at region offset %d: got %d, want %d" % (
        bad.size, bad[0] - d0, got[bad[0]], want[bad[0]])


PLANE_ORACLE = {"subsample420": lambda p, c: orc.subsample_hv2(p, c.dw, c.dh), "subsample422": lambda p, c: orc.subsample_h2(p, c.dw, c.dh),
                "upsample422": lambda p, c: orc.supersample_h2(p), "upsample420": lambda p, c: orc.supersample_hv2(p),
                "crop_planes": lambda p, c: orc.crop_plane(p, c.dw, c.dh, c.x, c.y)}


def run_plane_case(ctx, dev, c, rng):
    """-> (the cells the case landed in, by its actual addresses; None or what differs)"""
    as_strided = np.lib.stride_tricks.as_strided
    s_base, d_base = (dev.src.data_ptr(), dev.dst.data_ptr()) if c.device else (0, 0)
    s0, d0 = start_for(s_base, c.src_off), start_for(d_base, c.dst_off)
    src = rng.integers(0, 256, size=s0 + (c.n_planes - 1) * c.src_ps + (c.sh - 1) * c.src_stride + c.sw + GUARD, dtype=np.uint8)
    want = np.full(d0 + (c.n_planes - 1) * c.dst_ps + (c.dh - 1) * c.dst_stride + c.dw + GUARD, FILL, np.uint8)
    for p in range(c.n_planes):
        plane = np.ascontiguousarray(as_strided(src[s0 + p * c.src_ps:], (c.sh, c.sw), (c.src_stride, 1)))
        as_strided(want[d0 + p * c.dst_ps:], (c.dh, c.dw), (c.dst_stride, 1))[...] = PLANE_ORACLE[c.entry](plane, c)
    kw = dict(n_planes=c.n_planes, src_stride=c.src_stride, dst_stride=c.dst_stride, src_plane_stride=c.src_ps, dst_plane_stride=c.dst_ps)
    if c.entry == "crop_planes":
        call = lambda s, d: ctx.crop_planes(s, c.sw, c.sh, c.x, c.y, d, c.dw, c.dh, **kw)
    else:
        call = lambda s, d: getattr(ctx, c.entry)(s, c.sw, c.sh, d, **kw)
    got = run(dev, c.device, src, s0, want, d0, call)
    # (host memory goes through the context's staging buffers: fresh device allocations, aligned)
    return case_cells(c, s_base + s0 if c.device else 0, d_base + d0 if c.device else 0), first_difference(got, want, d0)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(ENTRY_KERNEL))
def test_plane_op_every_selection_cell(gpu, entry):
    """B1: hvc_subsample420 / _subsample422 / _upsample422 / _crop_planes / _upsample420 in every cell of the launcher's and the
    lanes' choice; the whole destination buffer against the oracle"""
    ctx, dev = gpu
    rng = np.random.Generator(np.random.PCG64(list(ENTRY_KERNEL).index(entry)))
    hit, wrong = set(), []
    for c in b1_cases(entry):
        cells, diff = run_plane_case(ctx, dev, c, rng)
        hit |= {(cell, c.device, c.dh if entry != "upsample420" else c.sh, c.n_planes) for cell in cells}
        if diff:
            wrong.append((c, cells, diff))
    assert not wrong, "%d cases differ; the first: %s" % (len(wrong), wrong[:5])
    assert not missing(b1_required(entry), hit)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(ENTRY_KERNEL))
def test_plane_op_on_a_permuted_grid(gpu, entry):
    """B4: more than one group of 128 workgroups, so hvc::xcd_work's permuted branch and its remainder both run, with padded
    strides and planes that are no power-of-two number of workgroups"""
    ctx, dev = gpu
    rng = np.random.Generator(np.random.PCG64(40 + list(ENTRY_KERNEL).index(entry)))
    for device in (False, True):
        c = b4_case(entry, device)
        wgs = b4_workgroups(c)
        assert wgs == 17 and wgs & (wgs - 1) and wgs * c.n_planes == 153 and 153 > 128 and 153 % 128 == 25
        cells, diff = run_plane_case(ctx, dev, c, rng)
        assert cells[0] == ("x8" if entry == "upsample420" else "vec, ragged")     # (K2: the only form that is permuted)
        assert not diff, (c, diff)


def run_convert(ctx, dev, hvc, fi, fo, size_in, size_out, off, frames, want_frames, device, src_off, dst_off):
    """n frames through hvc_yuv_convert -> (routes, launches by the actual addresses, None or what differs)"""
    F = lambda f: f if isinstance(f, int) else hvc.hvc.YUV_FORMATS[f]
    assert frames.shape[1] == hvc.hvc.yuv_frame_bytes(F(fi), *size_in) and len(want_frames) == frames.shape[0] * hvc.hvc.yuv_frame_bytes(F(fo), *size_out)
    s_base, d_base = (dev.src.data_ptr(), dev.dst.data_ptr()) if device else (0, 0)
    s0, d0 = start_for(s_base, src_off), start_for(d_base, dst_off)
    src = np.concatenate([np.full(s0, 0x3C, np.uint8), frames.reshape(-1), np.full(GUARD, 0x3C, np.uint8)])
    want = np.concatenate([np.full(d0, FILL, np.uint8), np.frombuffer(want_frames, np.uint8), np.full(GUARD, FILL, np.uint8)])
    call = lambda s, d: ctx.yuv_convert(s, F(fi), size_in, d, F(fo), size_out, offset=off, n_frames=frames.shape[0])
    got = run(dev, device, src, s0, want, d0, call)
    routes, launches = convert_launches(fi, fo, size_in, size_out, off, s_base + s0 if device else 0, d_base + d0 if device else 0)
    return routes, launches, first_difference(got, want, d0)


@pytest.mark.gpu
def test_convert_same_size_every_pair_size_and_base(gpu):
    """B2: Oconv.main's loop body at the same size with no offset: the fused chroma kernels' and the packing kernels' vector and
    scalar bodies, the last-row clamp with one chroma row, and the direct / luma_direct / luma_in_place routing, on host memory
    and on device memory at aligned and misaligned bases; three frames a call"""
    import video_coding_amd as hvc
    ctx, dev = gpu
    rng = np.random.Generator(np.random.PCG64(202))
    hit, wrong = set(), []
    for fi, fo, size in itertools.product(FORMATS, FORMATS, B2_SIZES):
        frames = rng.integers(0, 256, size=(3, frame_bytes(fi, *size)), dtype=np.uint8)
        want = b"".join(orc.oconv_frame(f, fi, size, fo, size) for f in frames)
        for device, so, do in B2_BASES:
            routes, launches, diff = run_convert(ctx, dev, hvc, fi, fo, size, size, (0, 0), frames, want, device, so, do)
            hit |= {("route", r, device) for r in routes} | {(k, c, device) for k, cells in launches for c in cells}
            if diff:
                wrong.append((fi, fo, size, device, so, do, launches, diff))
    assert not wrong, "%d cases differ; the first: %s" % (len(wrong), wrong[:5])
    assert not missing(b2_required(), hit)


@pytest.mark.gpu
def test_convert_with_a_crop_on_device_memory(gpu):
    """B3: the crop window read in place by the sub-sampling kernels (ragged and whole sub-sampled rows), the materialised crop,
    a negative offset and an output larger than the source, to 4:2:0, 4:2:2 and a packed format, on device memory at aligned
    and misaligned bases; two frames a call"""
    import video_coding_amd as hvc
    ctx, dev = gpu
    rng = np.random.Generator(np.random.PCG64(203))
    hit, wrong = set(), []
    for fi, fo, (size_in, size_out, off) in itertools.product(FORMATS, B3_OUTPUTS, B3_GEOMETRIES):
        frames = rng.integers(0, 256, size=(2, frame_bytes(fi, *size_in)), dtype=np.uint8)
        want = b"".join(orc.oconv_frame(f, fi, size_in, fo, size_out, off) for f in frames)
        for so, do in B3_BASES:
            routes, launches, diff = run_convert(ctx, dev, hvc, fi, fo, size_in, size_out, off, frames, want, True, so, do)
            hit.add((b3_class(routes, size_in, size_out, off), fo))
            if diff:
                wrong.append((fi, fo, size_in, size_out, off, so, do, launches, diff))
    assert not wrong, "%d cases differ; the first: %s" % (len(wrong), wrong[:5])
    assert not missing(set(itertools.product(B3_CLASSES, B3_OUTPUTS)), hit)
