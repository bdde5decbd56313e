"""The XCD workgroup order (csrc/hvc_kernels.h xcd_work / xcd_map_for) restated for the tests: which launches run permuted,
how a grid splits into the permuted part and the remainder, and the grid of every launch that takes its (frame, tile) from
xcd_work.  tests/test_xcd_grids.py holds the table of GPU tests that run each kernel family on such a grid;
tests/test_gpu_xcd_order.py takes its geometries from here, so the table describes what the GPU tests really launch.

Nothing here needs a GPU or the library."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 256          # HVC_TILE: blocks per workgroup of the tile kernels
MIXED_UNIT = 64     # HVC_MIXED_UNIT: blocks per work unit of the mixed kernels
MIXED_GROUP = 4     # HVC_MIXED_GROUP: units per workgroup
XCDS = 8


def source(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def default_runs():
    """(run, run of the fused 4:4:4 kernel): the defaults of xcd_map_run, from the text of csrc/hvc_kernels.h"""
    src = source("video-coding_amd", "csrc", "hvc_kernels.h")
    body = src[src.index("inline int xcd_map_run("):src.index("#ifdef __HIPCC__", src.index("inline int xcd_map_run("))]
    fused = re.search(r"if \(fused\) return run444 >= 0 \? run444 : run >= 0 \? run : (\d+);", body)
    plain = re.search(r"\n\s*return run >= 0 \? run : (\d+);", body)
    assert fused and plain, "xcd_map_run no longer reads as this helper restates it"
    return int(plain.group(1)), int(fused.group(1))


def xcd_map_for(per, n, fused=False):
    """the host's decision: 0 = workgroups as dispatched, else log2(run) + 1"""
    run = default_runs()[1 if fused else 0]
    if run <= 0 or per <= 1 or per * n * per >= 1 << 32:
        return 0
    sh = 0
    while (1 << (sh + 1)) <= run:
        sh += 1
    return sh + 1


def split(per, n, fused=False):
    """a grid of per x n workgroups -> dict(per, n, map, group, total, full (the permuted workgroups), rest (as dispatched))"""
    m = xcd_map_for(per, n, fused)
    total = per * n
    group = XCDS << (m - 1) if m else 0
    full = total - total % group if m else 0
    return dict(per=per, n=n, map=m, group=group, total=total, full=full, rest=total - full)


def replay(per, n, fused=False):
    """xcd_work for every workgroup of the grid, with the kernel's integer steps in 32 bits -> (frame, tile) arrays indexed by
    the workgroup's id = blockIdx.y * per + blockIdx.x"""
    s = split(per, n, fused)
    u32 = np.uint64(0xFFFFFFFF)
    ids = np.arange(s["total"], dtype=np.uint64)
    frame, tile = ids // np.uint64(per), ids % np.uint64(per)
    if s["map"]:
        sh = np.uint64(s["map"] - 1)
        magic = np.uint64(((1 << 32) + per - 1) // per)
        k = ids >> np.uint64(3)
        lin = ((((((k >> sh) << np.uint64(3)) + (ids & np.uint64(7))) & u32) << sh) & u32) + (k & ((np.uint64(1) << sh) - np.uint64(1)))
        lin &= u32
        f = (lin * magic) >> np.uint64(32)                      # __umulhi
        t = (lin - ((f * np.uint64(per)) & u32)) & u32
        inside = ids < np.uint64(s["full"])
        frame, tile = np.where(inside, f, frame), np.where(inside, t, tile)
    return frame.astype(np.int64), tile.astype(np.int64)


# ---- the grids of the launches ----------------------------------------------------------------------------------------
def tiles_per_frame(planes):
    """make_layout (csrc/hvc_capi.hip): every component's blocks in tiles of 256, a component's last tile ragged"""
    return sum(-(-bw * bh // TILE) for bw, bh, *_ in planes)


def mixed_units(frames):
    """mixed_plan_build: every plane with a block in units of 64, the frames' planes one after the other"""
    return sum(-(-bw * bh // MIXED_UNIT) for planes in frames for bw, bh, *_ in planes if bw * bh)


def mixed_groups(n_units):
    return -(-n_units // MIXED_GROUP)


def plan_decode_444(width, height, aligned=True):
    """plan_decode_444 (csrc/hvc_kernels.hip) for a 4:2:0 frame cropped to width x height -> dict(nw, y_tiles, c_tiles_x,
    c_tiles_y, tiles_per_frame); tile0 = 0 in the fused launch, so per = tiles_per_frame"""
    TILE_BW, TILE_BH = 64, 4
    y_cbw, y_cbh = -(-width // 8), -(-height // 8)
    cbw, cbh = -(-(width // 2) // 8), -(-(height // 2) // 8)
    nw = 1 if (not aligned or cbw <= TILE_BW) else 2 if cbw <= 2 * TILE_BW else 4
    wgs, tw = TILE * nw, TILE_BW * nw
    y_tiles = (y_cbw * y_cbh + wgs - 1) // wgs
    c_tiles_x = 1 if cbw <= tw else (cbw - 1 + (tw - 1) - 1) // (tw - 1)
    c_tiles_y = (cbh + TILE_BH - 1) // TILE_BH
    return dict(nw=nw, y_tiles=y_tiles, c_tiles_x=c_tiles_x, c_tiles_y=c_tiles_y, tiles_per_frame=y_tiles + 2 * c_tiles_x * c_tiles_y)


def upsample_x8_tiles(cw, ch):
    """launch_upsample420's wide form: a lane takes 8 source samples of a row"""
    return -(-(cw // 8) * ch // 256)


def plane_op_tiles(cols, rows):
    """launch_plane_op (csrc/hvc_yuv.hip): a lane takes 8 samples of a row"""
    return -(-(-(-cols // 8) * rows) // 256)


def packed_op_tiles(w, h):
    """launch_packed_op (csrc/hvc_yuv.hip): a lane takes 4 pairs of luma samples of a row"""
    return -(-((((w >> 1) + 3) >> 2) * h) // 256)


# ---- the geometries tests/test_gpu_xcd_order.py runs --------------------------------------------------------------------
# the tile kernels: 3 + 1 + 1 tiles a frame, the last luma tile ragged at 16 blocks; 29 frames = 145 workgroups = 128 + 17
TILE_PLANES = [(33, 16, 0), (9, 8, 1), (9, 8, 1)]
TILE_FRAMES = 29

# the files behind the GPU Huffman reader: 72 x 40 4:2:0 decodes to 80 x 48 / 40 x 24 / 40 x 24, one tile per component;
# 64 files in one chunk = 192 workgroups = 128 + 64
READER_SIZE = (72, 40)
READER_PLANES = [(10, 6, 0), (5, 3, 1), (5, 3, 1)]
READER_FILES = 64

# the mixed kernels: the frame shapes of the mixed modules' own `shapes` lists by name ...
MIXED_SHAPES = {
    "grey1": [(1, 1, 0)],                                    # one block
    "420": [(8, 8, 0), (4, 4, 1), (4, 4, 1)],                # planes of 64 / 16 / 16 blocks
    "444": [(9, 8, 0), (9, 8, 1), (9, 8, 1)],                # 72 blocks: a unit boundary
    "bw1": [(1, 257, 0)],                                    # bw = 1, five units
    "422": [(66, 33, 0), (33, 33, 1), (33, 33, 1)],          # 35 + 18 + 18 units
    "zero": [(4, 3, 0), (0, 3, 1), (2, 2, 1)],               # a zero-size component
}
# ... in an order that puts the one-block frame, the bw = 1 frame and the zero-size component inside the permuted part and a
# 4:2:2 frame across its end.  The first 18 frames are 480 units (6 x 71 + 1 + 5 + 2 + 6 + 3 + 37), so the seventh 4:2:2
# frame takes units 480 .. 550 = groups 120 .. 137, across group 128 where the remainder begins; 638 units in all = 160
# groups = 128 + 32, the last one with two spare units.  (test_xcd_grids.py asserts these places.)
MIXED_ORDER = ["422", "422", "grey1", "422", "bw1", "422", "zero", "422", "444", "422", "420", "444", "444", "420", "bw1", "bw1",
               "444", "444", "422", "444", "420", "grey1", "bw1", "grey1", "422"]
MIXED_BOUNDARY_FRAME = 18
# where a call takes no zero-size component: a one-block frame in its place (637 units, 160 groups, three spare units)
MIXED_ORDER_NO_ZERO = ["grey1" if name == "zero" else name for name in MIXED_ORDER]


def mixed_set(order):
    return [MIXED_SHAPES[name] for name in order]


def mixed_frame_groups(frames):
    """(first group, last group) of every frame of a mixed set"""
    out, u = [], 0
    for planes in frames:
        n = mixed_units([planes])
        out.append((u // MIXED_GROUP, (u + n - 1) // MIXED_GROUP if n else u // MIXED_GROUP))
        u += n
    return out
