"""The frame sets of tests/mixed_counts.py are what tests/test_gpu_mixed_counts.py claims of them: their group counts sit on
either side of the count at which xcd_map_for (csrc/hvc_kernels.h) switches the XCD workgroup order off, the replayed order is
a permutation there, a frame of many units lies across the end of the permuted part, and the blocks made to fail the int32
guard sit in the units named.  No GPU, no library: the restatement of xcd_work is tests/xcd_grids.py's."""
import ctypes as C

import numpy as np
import pytest

import mixed_counts as mc
import xcd_grids as xg

CASES = [(name, zero) for name in mc.UNITS for zero in (True, False)]


@pytest.mark.parametrize("name,zero", CASES)
def test_the_unit_and_group_counts(name, zero):
    s = mc.count_set(name, zero)
    frames = s.frames()
    assert xg.mixed_units(frames) == s.units == mc.UNITS[name]
    assert xg.mixed_groups(s.units) == s.groups == mc.GROUPS[name]
    spare = s.groups * xg.MIXED_GROUP - s.units
    assert spare == {"ON": 0, "ON_RAGGED": 2, "OFF": 2}[name]
    if name == "OFF":
        assert 262144 < s.units < 262148
    assert (s.units * xg.MIXED_UNIT >= 1 << 24) == (name == "OFF")  # the fix-up ids reach 2^24 - 256 / pass 2^24 by 128
    assert s.units * xg.MIXED_UNIT >= (1 << 24) - 512
    # the vectorised first units are those of xcd_grids
    groups = xg.mixed_frame_groups(frames)
    assert [g[0] for g in groups] == (s.unit0[:-1] // xg.MIXED_GROUP).tolist()
    assert [g[1] for g in groups] == ((s.unit0[1:] - 1) // xg.MIXED_GROUP).tolist()
    assert ("zero" in s.special.values()) == zero
    assert all(p[0] * p[1] > 0 for f in s.special for p in s.planes(f)) == (not zero)


@pytest.mark.parametrize("name", list(mc.UNITS))
def test_the_workgroup_order_at_the_edge(name):
    s = mc.count_set(name)
    sp = xg.split(s.groups, 1)
    if name == "OFF":                                              # 65537^2 >= 2^32: as dispatched
        assert xg.xcd_map_for(s.groups, 1) == 0 and (sp["full"], sp["rest"]) == (0, 65537)
    else:                                                          # 65535^2 < 2^32: the last permuted count
        assert xg.xcd_map_for(s.groups, 1) > 0 and sp["group"] == 128
        assert (sp["full"], sp["rest"]) == (mc.BOUNDARY_GROUP, 127)
    frame, tile = xg.replay(s.groups, 1)
    assert not frame.any()                                         # gridDim.y == 1: frame 0 throughout
    assert np.array_equal(np.sort(tile), np.arange(s.groups))      # every group once
    assert np.array_equal(tile[sp["full"]:], np.arange(sp["full"], s.groups))
    assert (np.count_nonzero(tile != np.arange(s.groups)) > 60000) == (name != "OFF")


def test_the_count_between_the_two_is_the_first_unpermuted():
    """65536 groups themselves: no set runs there (one side of the edge each is enough), the restatement agrees with the comment
    in launch_decode_mixed"""
    assert xg.xcd_map_for(mc.EDGE_GROUPS, 1) > 0 and xg.xcd_map_for(mc.EDGE_GROUPS + 1, 1) == 0
    magic = ((1 << 32) + mc.EDGE_GROUPS - 1) // mc.EDGE_GROUPS
    assert magic == 65538 and (mc.EDGE_GROUPS - 1) * magic == (1 << 32) - 4


@pytest.mark.parametrize("name,zero", CASES)
def test_where_the_frames_of_many_units_lie(name, zero):
    s = mc.count_set(name, zero)
    shapes = [s.special[f] for f in sorted(s.special)]
    assert shapes == ["422", "bw1", "zero" if zero else "grey1", "422", "grey1", "444"]
    assert s.unit0[0] == 0 and 0 in s.special                      # a 71-unit frame at unit 0
    b = s.boundary_frame
    first, last = s.unit0[b] // xg.MIXED_GROUP, (s.unit0[b + 1] - 1) // xg.MIXED_GROUP
    assert s.special[b] == "422" and first < mc.BOUNDARY_GROUP - 4 and last >= mc.BOUNDARY_GROUP + 4
    assert s.unit0[b] % xg.MIXED_GROUP != 0                        # (and it does not start a group)
    assert [f for f in s.special if s.unit0[f] // 4 < mc.BOUNDARY_GROUP <= (s.unit0[f + 1] - 1) // 4] == [b]
    assert s.n - 1 in s.special and s.unit0[s.n] == s.units        # the last frame ends the set
    if name == "OFF":                                              # ... and lies across group 65535 / 65536 there
        assert s.unit0[s.n - 1] // xg.MIXED_GROUP == 65535 and (s.units - 1) // xg.MIXED_GROUP == 65536
    runs = s.runs()
    assert sum(k for _, _, k in runs) == s.n and [f for kind, f, _ in runs if kind == "special"] == sorted(s.special)


@pytest.mark.parametrize("name", ["ON", "OFF"])
def test_where_the_guard_failing_blocks_sit(name):
    s = mc.count_set(name)
    where = [s.unit_of(*p) for p in s.guard_places()]
    edge = mc.BOUNDARY_GROUP * xg.MIXED_GROUP
    b_last = int(s.unit0[s.boundary_frame + 1]) - 1
    assert where == [(0, 5), (0, 63), (edge - 1, 63), (edge, 0), (b_last, 0), (s.units - 7, 0), (s.units - 1, 7)]
    assert (edge - 1) // xg.MIXED_GROUP == mc.BOUNDARY_GROUP - 1 and edge // xg.MIXED_GROUP == mc.BOUNDARY_GROUP
    ids = [u * xg.MIXED_UNIT + lane for u, lane in where]
    assert max(ids) == s.units * xg.MIXED_UNIT - 57 and len(set(ids)) == len(ids)
    assert (max(ids) >= 1 << 24) == (name == "OFF") and max(ids) >= (1 << 24) - 512
    assert all(f in s.special for f, _, _ in s.guard_places())     # records of their own: the tiled ones stay ordinary


def test_placement_and_fill():
    s = mc.count_set("ON_RAGGED")
    sizes = {f: 64 * sum(bw * bh for bw, bh, _ in s.planes(f)) for f in s.special}
    off, end = mc.place(s, 72, lambda f: sizes[f] + 3, align=8, lead=16)
    assert off[0] == 16 and (off % 8 == 0).all() and (np.diff(off) >= 72).all()
    assert end == 16 + 72 * (s.n - len(s.special)) + sum(-(-(v + 3) // 8) * 8 for v in sizes.values())
    out = np.full(end + 8, 0xA5, dtype=np.uint8)
    grey = (np.arange(mc.D * 64) % 199).astype(np.uint8).reshape(mc.D, 64)
    mc.fill(s, out, off, 72, lambda f: grey[f % mc.D], lambda f: np.full(sizes[f], f % 7, dtype=np.uint8))
    for f in (3, 70, 77, 250, 251, s.boundary_frame - 1, s.boundary_frame + 1, s.n - 3):
        assert f not in s.special
        assert np.array_equal(out[off[f]:off[f] + 64], grey[f % mc.D]) and (out[off[f] + 64:off[f] + 72] == 0xA5).all(), f
    for f in s.special:
        assert (out[off[f]:off[f] + sizes[f]] == f % 7).all() and out[off[f] + sizes[f]] == 0xA5
    assert (out[:16] == 0xA5).all() and (out[end:] == 0xA5).all()
    a = mc.size_array(off)
    assert len(a) == s.n and a[s.n - 1] == off[-1]


def test_descriptors_are_replicated_bytes():
    class Rec(C.Structure):
        _fields_ = [("a", C.c_int), ("t", (C.c_uint16 * 5) * 2), ("b", C.c_size_t)]
    s = mc.count_set("OFF")
    grey = [Rec(a=t, b=10 * t) for t in range(mc.TABLES)]
    for t in range(mc.TABLES):
        grey[t].t[1][4] = 100 + t
    arr = mc.descriptors(Rec, s, grey, lambda f: Rec(a=-f, b=f))
    assert len(arr) == s.n == 261996
    for f in (3, 4, 5, 77, 200000, s.n - 3):
        assert (arr[f].a, arr[f].t[1][4], arr[f].b) == (f % 3, 100 + f % 3, 10 * (f % 3)), f
    for f in s.special:
        assert (arr[f].a, arr[f].b) == (-f, f)


def test_the_files_for_the_table_set_cap():
    files, reusers = mc.table_set_files()
    assert len(files) == 528 and reusers == list(range(516, 524))
    first = [f for k, f in enumerate(files) if k not in reusers]
    assert len({mc.dht_payload(f) for f in first}) == 520 >= 516                 # every file its own table set
    for at, src in zip(reusers, mc.REUSERS):
        assert mc.dht_payload(files[at]) == mc.dht_payload(files[src]) and files[at] != files[src]
    # 516 distinct sets stand before the re-users: files 512 .. 515 are past the cap, the re-users' sets are inside it
    assert mc.beyond_the_table_sets(files) == [512, 513, 514, 515, 524, 525, 526, 527]
    assert mc.beyond_the_table_sets(files[:512]) == [] and mc.beyond_the_table_sets(files[:513]) == [512]
