"""tests/tiles444.py held to what it claims, on the CPU: every row of CASES is the plan its columns say, every block of a crop is
stored by exactly one lane, the host's inversion undoes locate444, the ids fit their range, and the rows together reach every
kind of plan that plan_decode_444 can produce.  tests/test_gpu_yuv444.py runs the rows on the device."""
import re

import pytest

import tiles444 as t4
import xcd_grids as xg

SIZES = sorted({(c.width, c.height, c.aligned) for c in t4.CASES} | {(w, h, w % 16 == 0) for w, h in t4.EXISTING})


def test_the_header_and_the_plan_agree_on_the_tile():
    """xg.plan_decode_444 carries the tile as numbers of its own: they are the header's"""
    bw, bh = t4.TILE_BW, t4.TILE_BH
    assert (bw, bh) == (64, 4)          # CASES was chosen for this tile: another one needs other sizes (the coverage test says which)
    assert [xg.plan_decode_444(16 * n, 16)["nw"] for n in (bw, bw + 1, 2 * bw, 2 * bw + 1)] == [1, 2, 2, 4]
    assert [xg.plan_decode_444(16, 16 * n)["c_tiles_y"] for n in (bh, bh + 1)] == [1, 2]
    src = xg.source("video-coding_amd", "csrc", "hvc_kernels.hip")
    body = src[src.index("void plan_decode_444("):src.index("template <bool ALIGNED, int NW>")]
    for line in ("P.nw = !aligned || cbw <= HVC_444_TILE_BW ? 1 : cbw <= 2 * HVC_444_TILE_BW ? 2 : 4;",
                 "P.c_tiles_x = cbw <= tw ? 1 : (cbw - 1 + (tw - 1) - 1) / (tw - 1);",
                 "P.c_tiles_y = (P.pl[1].cbh + HVC_444_TILE_BH - 1) / HVC_444_TILE_BH;"):
        assert line in body, "plan_decode_444 no longer reads as xcd_grids restates it: " + line


@pytest.mark.parametrize("case", t4.CASES, ids=lambda c: c.id)
def test_a_row_is_what_it_says(case):
    g = case.geometry()
    assert case.form == ("aligned" if case.aligned else "bytes") == g.kind()[0]
    assert (g.nw, g.cbw[1], (g.c_tiles_x, g.c_tiles_y)) == (case.nw, case.cbw, case.tiles)
    tx, lx, kind = g.last_column_owner()
    assert kind == case.owner
    # ... and the restated kernel agrees: in every tile row that lane, and no other, stores the last column
    for p in (1, 2):
        for ty in range(g.c_tiles_y):
            owners = []
            for x in range(g.c_tiles_x):
                tile = g.y_tiles + (p - 1) * g.c_tiles_x * g.c_tiles_y + ty * g.c_tiles_x + x
                for l in range(g.tw):
                    pp, bx, by, active, store = t4.locate444(g, tile, l)
                    if store and bx == g.cbw[p] - 1:
                        owners.append((x, l))
            assert owners == [(tx, lx)], (p, ty, owners)
    assert tx == g.c_tiles_x - 1 and (lx == g.tw - 1) == (kind != t4.ORDINARY) and (kind == t4.OVERLAP_LATER) == (lx == g.tw - 1 and tx > 0)
    if case.stride_extra != 64 or case.offset:      # the rows that take the byte form for the stride's or the pointer's sake
        assert case.width % 16 == 0 and not case.aligned
        assert (case.frame_stride % 16 == 0) == bool(case.offset)


@pytest.mark.parametrize("width,height,aligned", SIZES)
def test_every_block_of_the_crop_is_stored_once_and_found_again(width, height, aligned):
    g = t4.Geometry(width, height, aligned)
    assert g.tiles_per_frame == g.y_tiles + 2 * g.c_tiles_x * g.c_tiles_y
    stored, active_in = {}, {}
    ids = set()
    for tile in range(g.tiles_per_frame):
        for lane in range(g.wgs):
            p, bx, by, active, store = t4.locate444(g, tile, lane)
            assert 0 <= bx < g.cbw[p] and 0 <= by < g.cbh[p]          # (clamped: even an idle lane reads inside the crop)
            assert not store or active
            if active:
                active_in[p, bx, by] = active_in.get((p, bx, by), 0) + 1
            if store:
                stored[p, bx, by] = stored.get((p, bx, by), 0) + 1
                assert t4.tile_lane_of(g, p, bx, by) == (tile, lane)  # the host finds the storing lane, nobody else
                for frame in (0, 1):
                    ident = t4.fix_id(g, frame, tile, lane)
                    assert ident < 2 * g.tiles_per_frame * xg.TILE * g.nw and t4.split_id(g, ident) == (frame, tile, lane)
                    ids.add(ident)
    blocks = {(p, bx, by) for p in range(3) for by in range(g.cbh[p]) for bx in range(g.cbw[p])}
    assert set(stored) == blocks and set(stored.values()) == {1}
    assert len(ids) == 2 * len(blocks)
    assert max(ids) < 2 * g.tiles_per_frame * xg.TILE * g.nw
    shared = set(g.shared_columns())
    assert all(0 < s < g.cbw[1] - 1 for s in shared) and len(shared) == g.c_tiles_x - 1
    for (p, bx, by), n in active_in.items():
        assert n == (2 if p and bx in shared else 1), (p, bx, by, n)
    # the other way round: every block of the crop comes back from its (tile, lane), the last column through the clamp
    for p, bx, by in blocks:
        tile, lane = t4.tile_lane_of(g, p, bx, by)
        assert t4.locate444(g, tile, lane) == (p, bx, by, True, True)


def test_the_rows_reach_every_kind_of_plan():
    """every (store form, nw, tiles across, owner of the last column) that a chroma crop of 1 .. 800 blocks can be given:
    none without a row.  (The plan takes nothing from the frame but cbw and the form, so these are all there are up to three
    tiles of the widest kind across.)"""
    possible = {}
    for cbw in range(1, 801):
        for aligned in (True, False):
            possible.setdefault(t4.Geometry(16 * cbw, 16, aligned).kind(), cbw)
    assert {k[1] for k in possible} == {1, 2, 4} and {k[3] for k in possible} == {t4.ORDINARY, t4.OVERLAP_FIRST, t4.OVERLAP_LATER}
    assert {k[2] for k in possible if k[0] == "aligned"} == {1, 2, 3} == {k[2] for k in possible if k[0] == "bytes"}
    covered = {c.geometry().kind() for c in t4.CASES}
    missing = {k: cbw for k, cbw in possible.items() if k not in covered}
    assert not missing, "no row of CASES for (form, nw, tiles across, owner): first cbw %r" % missing
    assert covered <= set(possible)


def test_the_wide_rows_take_the_split_launch_too():
    """decode_frames_yuv444_impl's condition for HVC_444_MODE=1 / 2 (16-byte form, height % 8 == 0, the luma crop the whole
    plane): the rows with two and three NW = 4 tiles across meet it, so the child runs of test_gpu_yuv444 take them with the
    chroma tiles alone (tile0 = y_tiles)"""
    split = [c for c in t4.CASES if c.aligned and c.height % 8 == 0 and c.geometry().cbw[0] == (c.width + 15) // 16 * 2]
    assert {(c.width, c.height) for c in split} >= {(8176, 32), (8192, 80), (12256, 32)}
    assert {c.geometry().kind()[1:] for c in split} >= {(4, 2, t4.OVERLAP_LATER), (4, 3, t4.ORDINARY), (4, 3, t4.OVERLAP_LATER)}


def test_the_earlier_sizes_are_still_run():
    src = xg.source("tests", "test_gpu_yuv444.py")
    for w, h in t4.EXISTING:
        assert re.search(r"\(%d, %d\)|width, height = %d, %d\b" % (w, h, w, h), src), (w, h)
