"""The tile plan of the fused 4:4:4 decode restated for the tests, on top of xcd_grids.plan_decode_444: which block a lane of a
tile decodes and whether it stores it (locate444, csrc/hvc_kernels.hip), the host's way back from a chroma block to its (tile,
lane) (apply_wide_dc_444, csrc/hvc_capi.hip), and the fix-up id (frame * tiles_per_frame + tile) * 256 * nw + lane that
k_decode_444 writes and k_decode_wide_444, k_reinterp_444, launch_decode_444_dcfix and apply_wide_dc_444 read.

CASES is the table of sizes that tests/test_gpu_yuv444.py runs for the plan's sake; tests/test_tiles444.py holds every row to
what it claims, on the CPU, and proves that the rows together reach every kind of plan there is.

Nothing here needs a GPU or the library."""
import re

import xcd_grids as xg


def header_constants():
    """HVC_444_TILE_BW / HVC_444_TILE_BH from the text of csrc/hvc_kernels.h"""
    src = xg.source("video-coding_amd", "csrc", "hvc_kernels.h")
    bw = re.search(r"^#define HVC_444_TILE_BW (\d+)\s*$", src, re.M)
    bh = re.search(r"^#define HVC_444_TILE_BH (\d+)\s*$", src, re.M)
    assert bw and bh, "hvc_kernels.h no longer defines the 4:4:4 tile as this helper reads it"
    return int(bw.group(1)), int(bh.group(1))


TILE_BW, TILE_BH = header_constants()

ORDINARY, OVERLAP_FIRST, OVERLAP_LATER = "ordinary lane", "overlap lane of tile 0", "overlap lane of a later tile"


class Geometry:
    """A 4:2:0 frame cropped to width x height, in the form that decode_frames_yuv444_impl hands to plan_decode_444.
    aligned: the 16-byte store form (width, frame stride and output pointer all multiples of 16).
    cbw / cbh [plane]: the blocks that intersect the crop; aw / ah [plane]: the crop in samples."""

    def __init__(self, width, height, aligned=None):
        self.width, self.height = width, height
        self.aligned = width % 16 == 0 if aligned is None else aligned
        assert not self.aligned or width % 16 == 0
        self.aw, self.ah = [width, width // 2, width // 2], [height, height // 2, height // 2]
        self.cbw, self.cbh = [-(-a // 8) for a in self.aw], [-(-a // 8) for a in self.ah]
        plan = xg.plan_decode_444(width, height, self.aligned)
        self.nw, self.y_tiles, self.c_tiles_x, self.c_tiles_y = plan["nw"], plan["y_tiles"], plan["c_tiles_x"], plan["c_tiles_y"]
        self.tiles_per_frame = plan["tiles_per_frame"]
        self.wgs, self.tw = xg.TILE * self.nw, TILE_BW * self.nw
        self.c_magic = ((1 << 32) + self.c_tiles_x - 1) // self.c_tiles_x
        self.y_magic = ((1 << 32) + self.cbw[0] - 1) // self.cbw[0]

    def shared_columns(self):
        """the chroma block columns that two tiles of a row decode: tile k's lane tw - 1 and tile k + 1's lane 0"""
        return [k * (self.tw - 1) for k in range(1, self.c_tiles_x)]

    def last_column_owner(self):
        """(tx, lx, kind) of the lane that stores chroma block column cbw - 1"""
        lanes = [(tx, self.cbw[1] - 1 - tx * (self.tw - 1)) for tx in range(self.c_tiles_x)]
        # (a column that two tiles held would belong to the later one's lane 0: the last tile that reaches it)
        tx, lx = [(tx, lx) for tx, lx in lanes if 0 <= lx < self.tw][-1]
        return tx, lx, ORDINARY if lx < self.tw - 1 else OVERLAP_FIRST if tx == 0 else OVERLAP_LATER

    def kind(self):
        """what test_tiles444's coverage claim counts: (form, nw, tiles across as 1 / 2 / 3 = three or more, last column's owner)"""
        return ("aligned" if self.aligned else "bytes", self.nw, min(self.c_tiles_x, 3), self.last_column_owner()[2])


def umulhi(a, b):
    return (a * b) >> 32


def locate444(g, tile, lane):
    """locate444 -> (plane, bx, by, active, store); bx / by clamped into the crop as the kernel clamps them"""
    if tile < g.y_tiles:
        n = g.cbw[0] * g.cbh[0]
        b = tile * g.wgs + lane
        active = b < n
        b = b if active else n - 1
        by = b if g.cbw[0] == 1 else umulhi(b, g.y_magic)
        return 0, b - by * g.cbw[0], by, active, active
    t, per, p = tile - g.y_tiles, g.c_tiles_x * g.c_tiles_y, 1
    if t >= per:
        p, t = 2, t - per
    ty = t if g.c_tiles_x == 1 else umulhi(t, g.c_magic)
    tx = t - ty * g.c_tiles_x
    lx, ly = lane & (g.tw - 1), lane // g.tw
    bx, by = tx * (g.tw - 1) + lx, ty * TILE_BH + ly
    active = bx < g.cbw[p] and by < g.cbh[p]
    store = active and (lx < g.tw - 1 or bx == g.cbw[p] - 1)
    return p, min(bx, g.cbw[p] - 1), min(by, g.cbh[p] - 1), active, store


def tile_lane_of(g, p, bx, by):
    """apply_wide_dc_444: the (tile, lane) whose id makes the kernels rewrite block (bx, by) of plane p"""
    if p == 0:
        b = by * g.cbw[0] + bx
        return b // g.wgs, b % g.wgs
    tx = 0 if g.c_tiles_x == 1 else bx // (g.tw - 1)
    if tx >= g.c_tiles_x:      # the last column where it is the last tile's overlap lane
        tx = g.c_tiles_x - 1
    lx, ty, ly = bx - tx * (g.tw - 1), by // TILE_BH, by % TILE_BH
    return g.y_tiles + (p - 1) * g.c_tiles_x * g.c_tiles_y + ty * g.c_tiles_x + tx, ly * g.tw + lx


def fix_id(g, frame, tile, lane):
    return (frame * g.tiles_per_frame + tile) * xg.TILE * g.nw + lane


def split_id(g, ident):
    """the readers' way back: id -> (frame, tile, lane)"""
    lane, t = ident % g.wgs, ident // g.wgs
    return t // g.tiles_per_frame, t % g.tiles_per_frame, lane


class Case:
    """One row of CASES.  stride_extra: bytes between the frames of a batch behind each frame's 3 * width * height;
    offset: bytes by which the device output is moved off its allocation; the claims nw / cbw / tiles (across, down) / owner
    are what tests/test_tiles444.py checks against the plan."""

    def __init__(self, width, height, form, nw, cbw, tiles, owner, why, stride_extra=64, offset=0):
        self.width, self.height, self.form, self.nw, self.cbw, self.tiles, self.owner, self.why = width, height, form, nw, cbw, tiles, owner, why
        self.stride_extra, self.offset = stride_extra, offset

    @property
    def frame_stride(self):
        return 3 * self.width * self.height + self.stride_extra

    @property
    def aligned(self):
        """launch_decode_444's own test on what the call is given"""
        return self.width % 16 == 0 and self.frame_stride % 16 == 0 and self.offset % 16 == 0

    def geometry(self):
        return Geometry(self.width, self.height, self.aligned)

    @property
    def id(self):
        return "%dx%d%s%s" % (self.width, self.height, "+stride%d" % self.stride_extra if self.stride_extra != 64 else "",
                              "+offset%d" % self.offset if self.offset else "")


CASES = [
    # ---- one tile across at every tile width --------------------------------------------------------------------------
    Case(80, 16, "aligned", 1, 5, (1, 1), ORDINARY, "a narrow tile whose last column is an ordinary lane"),
    Case(1024, 16, "aligned", 1, 64, (1, 1), OVERLAP_FIRST, "lane 63 owns the last column"),
    Case(1040, 16, "aligned", 2, 65, (1, 1), ORDINARY, "first width of NW = 2"),
    Case(2048, 32, "aligned", 2, 128, (1, 1), OVERLAP_FIRST, "lane 127 owns the last column"),
    Case(2064, 32, "aligned", 4, 129, (1, 1), ORDINARY, "first width of NW = 4"),
    Case(4096, 32, "aligned", 4, 256, (1, 1), OVERLAP_FIRST, "lane 255 owns the last column"),
    # ---- more than one tile across with 16-byte stores: only NW = 4 gets there ----------------------------------------
    Case(4112, 66, "aligned", 4, 257, (2, 2), ORDINARY,
         "second tile holds columns 255 and 256; ah = 33, so the lower tile row holds one sample row (lasty == 0) under a seam"),
    Case(8176, 32, "aligned", 4, 511, (2, 1), OVERLAP_LATER, "510 = 2 * 255: the last column is tile 1's overlap lane"),
    Case(8192, 80, "aligned", 4, 512, (3, 2), ORDINARY, "three tiles across, a seam, c_magic with divisor 3"),
    Case(12256, 32, "aligned", 4, 766, (3, 1), OVERLAP_LATER, "765 = 3 * 255: the last column is tile 2's overlap lane"),
    # ---- the byte-store form ---------------------------------------------------------------------------------------------
    Case(50, 6, "bytes", 1, 4, (1, 1), ORDINARY, "one narrow tile, aw = 25 ends inside a block, ah = 3"),
    Case(1022, 18, "bytes", 1, 64, (1, 1), OVERLAP_FIRST, "lane 63 owns a partial last column"),
    Case(1026, 18, "bytes", 1, 65, (2, 1), ORDINARY, "the second tile holds columns 63 and 64, the last one with a single sample"),
    Case(2030, 34, "bytes", 1, 127, (2, 1), OVERLAP_LATER,
         "126 = 2 * 63: overlap-lane owner in the byte form, aw = 1015 ends inside a block, ah = 17"),
    Case(3038, 18, "bytes", 1, 190, (3, 1), OVERLAP_LATER, "189 = 3 * 63: tile 2's overlap lane owns a partial last column"),
    Case(2080, 80, "bytes", 1, 130, (3, 2), ORDINARY, "aligned width, unaligned stride", stride_extra=8),
    Case(2080, 80, "bytes", 1, 130, (3, 2), ORDINARY, "aligned width and stride, unaligned pointer", offset=8),
]

# the sizes tests/test_gpu_yuv444.py ran before CASES (its parametrisations and the sizes inside its tests), all with a tight
# stride into a fresh allocation; tests/test_tiles444.py checks the plan's properties on them too and that they are still there
EXISTING = [(64, 48), (64, 40), (1056, 144), (2080, 80), (1024, 32), (1040, 32), (2032, 32), (48, 272), (1920, 1080),
            (52, 44), (100, 30), (18, 10), (2, 2), (1042, 70), (24, 8), (64, 32), (80, 48), (1056, 80), (48, 32)]
