"""Which GPU test runs which kernel family under the XCD workgroup order (csrc/hvc_kernels.h xcd_work).  A launch below one
group of 8 x R workgroups runs entirely as dispatched, so a parity test on a small grid says nothing about the branch every
production-size batch takes.  The table names, for every family that takes its (frame, tile) from xcd_work, one GPU test
and the grid it launches; the grid must be permuted, with a remainder, across frames and components.  A GPU test that
shrinks below that, or a changed default run length, fails here."""
import numpy as np
import pytest

import mixed_counts as mc
import xcd_grids as xg

TILE_GRID = dict(per=xg.tiles_per_frame(xg.TILE_PLANES), n=xg.TILE_FRAMES, parts=len(xg.TILE_PLANES))
READER_GRID = dict(per=xg.tiles_per_frame(xg.READER_PLANES), n=xg.READER_FILES, parts=len(xg.READER_PLANES))


def mixed_grid(order):
    frames = xg.mixed_set(order)
    units = xg.mixed_units(frames)
    return dict(per=xg.mixed_groups(units), n=1, units=units, frames=len(frames), parts=max(len(p) for p in frames))


MIXED_GRID = mixed_grid(xg.MIXED_ORDER)
MIXED_GRID_NO_ZERO = mixed_grid(xg.MIXED_ORDER_NO_ZERO)
FUSED_GRID = dict(per=xg.plan_decode_444(1920, 1080)["tiles_per_frame"], n=12, parts=3, fused=True)
UPSAMPLE_GRID = dict(per=xg.upsample_x8_tiles(960, 540), n=4, parts=4)          # grid.y = the planes
B4_GRID = dict(per=xg.plane_op_tiles(260, 131), n=9, parts=9)
B4_GRID_K2 = dict(per=xg.upsample_x8_tiles(264, 131), n=9, parts=9)
# hvc_yuv_convert at 1920 x 1080, two frames a call (host memory: the call uploads both and launches once): grid.y = the frames
PACKED_GRID = dict(per=xg.packed_op_tiles(1920, 1080), n=2, parts=3)
CHROMA_GRID = dict(per=xg.plane_op_tiles(960, 540), n=2, parts=2)               # the u and the v plane, a launch each


def count_grid(name, zero=True):
    """a set of tests/mixed_counts.py: at 65535 groups the last permuted launch, at 65537 the launch as dispatched"""
    s = mc.count_set(name, zero)
    return dict(per=s.groups, n=1, units=s.units, frames=s.n, parts=3, edge=name)


NEW = "test_gpu_xcd_order.py"
COUNTS = "test_gpu_mixed_counts.py"
# (kernel family, test module, test function, grid, text the test's source must hold: its geometry)
TABLE = [
    ("k_decode_packed<false>", NEW, "test_decode_frames_model", TILE_GRID, ()),
    ("k_decode_packed<false> + k_decode_wide (fix-up ids)", NEW, "test_decode_frames_model_blocks_outside_the_guard", TILE_GRID, ()),
    ("k_decode_wide_all", NEW, "test_decode_frames_every_block_wide", TILE_GRID, ()),
    ("k_hardcaml", NEW, "test_decode_frames_hardcaml", TILE_GRID, ()),
    ("k_islow<false>", NEW, "test_decode_frames_libjpeg", TILE_GRID, ()),
    ("k_decode_scaled<N, false, DW>", NEW, "test_decode_frames_scaled", TILE_GRID, ()),
    ("k_encode", NEW, "test_encode_frames_model", TILE_GRID, ()),
    ("k_hardcaml_encode", NEW, "test_encode_frames_hardcaml", TILE_GRID, ()),
    ("k_decode_mixed", NEW, "test_decode_frames_mixed", MIXED_GRID, ()),
    ("k_decode_mixed + k_decode_mixed_wide (fix-up ids)", NEW, "test_decode_frames_mixed_blocks_outside_the_guard", MIXED_GRID, ()),
    ("k_decode_mixed_scaled<N>", NEW, "test_decode_frames_mixed_scaled", MIXED_GRID, ()),
    ("k_encode_mixed", NEW, "test_encode_frames_mixed", MIXED_GRID_NO_ZERO, ()),
    ("k_islow_mixed", NEW, "test_decode_frames_mixed_libjpeg", MIXED_GRID_NO_ZERO, ()),
    ("k_decode_packed<true>", NEW, "test_gpu_reader_batch_model", READER_GRID, ()),
    ("k_islow<true>", NEW, "test_gpu_reader_batch_libjpeg", READER_GRID, ()),
    ("k_decode_scaled<N, true, DW>", NEW, "test_gpu_reader_batch_scaled", READER_GRID, ()),
    ("k_decode_444", "test_gpu_yuv444.py", "test_equals_the_separate_kernels_at_full_size", FUSED_GRID,
     ("width, height = 1920, 1080", "n = 12", "ctx.decode_frames_yuv444(d_c, cfs, qt, specs, n, width, height, d_o)")),
    ("k_upsample420_x8", "test_gpu_encode_upsample.py", "test_upsample_wide_variant_and_strides", UPSAMPLE_GRID,
     ("(960, 540, 960, 1920)", "n = 4", "n_planes=n")),
    ("hvc_yuv.hip: k_subsample420, k_subsample422, k_upsample422, k_crop", "test_gpu_yuv_paths.py", "test_plane_op_on_a_permuted_grid",
     B4_GRID, ("make_case(entry, 264 if entry == \"upsample420\" else 260, 131, 9, device)",)),
    ("k_upsample420_x8 (through the plane-operation entry point)", "test_gpu_yuv_paths.py", "test_plane_op_on_a_permuted_grid",
     B4_GRID_K2, ("make_case(entry, 264 if entry == \"upsample420\" else 260, 131, 9, device)",)),
    ("hvc_yuv.hip: k_unpack422, k_pack422", "test_gpu_yuv_convert.py", "test_oconv_pipeline_every_format_pair", PACKED_GRID,
     ("((1920, 1080), (1920, 1080), (0, 0))", "(\"YVYU\", \"YUY2\")", "n_frames=2")),
    ("hvc_yuv.hip: k_chroma_420_to_422, k_chroma_422_to_420", "test_gpu_yuv_convert.py", "test_oconv_pipeline_every_format_pair", CHROMA_GRID,
     ("((1920, 1080), (1920, 1080), (0, 0))", "(420, \"UYVY\")", "(\"YUY2\", 420)", "n_frames=2")),
    # the four mixed families at the counts where the order is switched off (tests/mixed_counts.py): 65535 groups, the last
    # one full (ON) and ragged (ON_RAGGED), and 65537 groups (OFF)
    ("k_decode_mixed", COUNTS, "test_decode_frames_mixed", count_grid("ON"), ('["ON", "ON_RAGGED", "OFF"]',)),
    ("k_decode_mixed", COUNTS, "test_decode_frames_mixed", count_grid("ON_RAGGED"), ('["ON", "ON_RAGGED", "OFF"]',)),
    ("k_decode_mixed", COUNTS, "test_decode_frames_mixed", count_grid("OFF"), ('["ON", "ON_RAGGED", "OFF"]',)),
    ("k_decode_mixed + k_decode_mixed_wide (fix-up ids)", COUNTS, "test_decode_frames_mixed_fix_up_ids", count_grid("ON"), ()),
    ("k_decode_mixed + k_decode_mixed_wide (fix-up ids)", COUNTS, "test_decode_frames_mixed_fix_up_ids", count_grid("OFF"), ()),
    ("k_decode_mixed_scaled<N>", COUNTS, "test_decode_frames_mixed_scaled", count_grid("ON"), ()),
    ("k_decode_mixed_scaled<N>", COUNTS, "test_decode_frames_mixed_scaled", count_grid("OFF"), ()),
    ("k_encode_mixed", COUNTS, "test_encode_frames_mixed", count_grid("ON", False), ()),
    ("k_encode_mixed", COUNTS, "test_encode_frames_mixed", count_grid("OFF", False), ()),
    ("k_islow_mixed", COUNTS, "test_decode_frames_mixed_libjpeg", count_grid("ON", False), ()),
    ("k_islow_mixed", COUNTS, "test_decode_frames_mixed_libjpeg", count_grid("OFF", False), ()),
]
FAMILIES = ("k_decode_packed<false>", "k_decode_packed<true>", "k_decode_wide_all", "k_decode_444", "k_encode", "k_upsample420_x8",
            "k_hardcaml", "k_hardcaml_encode", "k_islow<false>", "k_islow<true>", "k_decode_scaled<N, false, DW>",
            "k_decode_scaled<N, true, DW>", "k_decode_mixed", "k_decode_mixed_scaled<N>", "k_encode_mixed", "k_islow_mixed",
            "hvc_yuv.hip: k_subsample420, k_subsample422, k_upsample422, k_crop", "hvc_yuv.hip: k_unpack422, k_pack422",
            "hvc_yuv.hip: k_chroma_420_to_422, k_chroma_422_to_420")


def test_the_default_run_lengths_are_the_ones_the_table_was_made_for():
    assert xg.default_runs() == (16, 64)
    assert xg.split(5, 29)["group"] == 128 and xg.split(98, 12, fused=True)["group"] == 512


def test_every_family_runs_permuted_with_a_remainder_in_a_gpu_test():
    assert set(FAMILIES) <= {row[0] for row in TABLE}
    report = []
    for family, module, test, grid, texts in TABLE:
        src = xg.source("tests", module)
        assert "def %s(" % test in src, (family, module, test)
        for t in texts:                                    # the existing test still has the geometry this row restates
            assert t in src, (family, t)
        if module == NEW:                                  # the new tests take theirs from xcd_grids, by these names
            for name in ("xg.TILE_PLANES", "xg.TILE_FRAMES", "xg.MIXED_ORDER", "xg.MIXED_ORDER_NO_ZERO", "xg.READER_FILES", "xg.READER_SIZE"):
                assert name in src, name
        if module == COUNTS:                               # ... and these theirs from mixed_counts
            assert "mc.count_set(name" in src and '@pytest.mark.parametrize("name", ["ON", "OFF"])' in src
        per, n, fused = grid["per"], grid["n"], grid.get("fused", False)
        s = xg.split(per, n, fused)
        report.append((family, per, n, s["full"], s["rest"]))
        if grid.get("edge") == "OFF":                      # past the switch: nothing is permuted, every group runs once
            assert per == 65537 and s["map"] == 0 and (s["full"], s["rest"]) == (0, per), family
            frame, tile = xg.replay(per, n, fused)
            assert not frame.any() and np.array_equal(tile, np.arange(per)), family
            assert grid["units"] % xg.MIXED_GROUP != 0 and grid["frames"] > 1, family
            continue
        assert s["map"] > 0, family                                                    # (a) the mapping is on
        assert s["full"] >= s["group"] > 0, family                                     # (b) a whole group is permuted
        assert s["rest"] > 0, family                                                   # (c) a remainder as dispatched
        if "edge" in grid:                                                             # (d) the last count that is permuted
            assert per == 65535 and xg.xcd_map_for(per + 1, 1) == 0, family
            assert (grid["units"] % xg.MIXED_GROUP != 0) == (grid["edge"] == "ON_RAGGED"), family
            assert grid["frames"] > 1 and grid["parts"] > 1, family                    # (e)
        elif "units" in grid:                                                          # (d) ragged against the run length
            assert grid["units"] % xg.MIXED_GROUP != 0, family                         #     ... the last group has spare units
            assert 513 <= grid["units"] <= 1020, family
            assert grid["frames"] > 1 and grid["parts"] > 1, family                    # (e)
        else:
            assert per & (per - 1) != 0, family
            assert n > 1 and grid["parts"] > 1, family                                 # (e) frames and components (or planes)
        frame, tile = xg.replay(per, n, fused)                                         # (f) workgroups that leave their place
        ids = np.arange(per * n)
        assert np.array_equal(np.sort(frame * per + tile), ids), family                #     (and still a permutation)
        assert np.array_equal((frame * per + tile)[s["full"]:], ids[s["full"]:]), family
        if "units" in grid:
            assert np.count_nonzero((frame * per + tile)[:s["full"]] != ids[:s["full"]]) > 0, family
        else:
            assert np.count_nonzero(frame[:s["full"]] != ids[:s["full"]] // per) > 0, family
    for line in report:
        print("%-70s per %5d  n %3d  permuted %5d  remainder %5d" % line)


def test_the_tile_geometry_is_the_one_the_issue_of_this_table_describes():
    assert TILE_GRID["per"] == 5 and xg.TILE_PLANES[0][0] * xg.TILE_PLANES[0][1] % xg.TILE == 16   # the last luma tile: 16 blocks
    s = xg.split(5, xg.TILE_FRAMES)
    assert (s["total"], s["full"], s["rest"]) == (145, 128, 17)
    r = xg.split(READER_GRID["per"], xg.READER_FILES)
    assert (READER_GRID["per"], r["total"], r["full"], r["rest"]) == (3, 192, 128, 64)


@pytest.mark.parametrize("order", [xg.MIXED_ORDER, xg.MIXED_ORDER_NO_ZERO], ids=["with_zero", "without_zero"])
def test_the_mixed_set_puts_its_small_frames_inside_the_permuted_part(order):
    frames = xg.mixed_set(order)
    groups = xg.mixed_frame_groups(frames)
    full = xg.split(xg.mixed_groups(xg.mixed_units(frames)), 1)["full"]
    assert full == 128
    for name in ("grey1", "bw1", "zero"):
        if name in order:
            assert groups[order.index(name)][1] < full, name                           # wholly inside the permuted part
    first, last = groups[xg.MIXED_BOUNDARY_FRAME]
    assert order[xg.MIXED_BOUNDARY_FRAME] == "422" and first < full - 4 and last >= full + 4   # across the boundary
    assert len({name for name in order}) >= 5
