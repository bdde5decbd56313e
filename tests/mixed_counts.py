"""Frame sets with an exact number of work units for the mixed kernels, at the counts where their indexing changes: the XCD
workgroup order is used up to 65535 groups and switched off from 65536 (csrc/hvc_kernels.h xcd_map_for: groups^2 < 2^32), and
the fix-up ids unit * 64 + lane of k_decode_mixed reach 2^24 there.  tests/test_gpu_mixed_counts.py runs the sets;
tests/test_mixed_counts.py holds them to what that module claims of them, on the CPU.  The geometry helpers are those of
tests/xcd_grids.py.

A set is one-block grey frames (xg.MIXED_SHAPES["grey1"]: one unit each) with a few frames of several units at chosen units:
at unit 0, across group 65408 (where the permuted part of a 65535-group launch ends) and as the last frame.  Grey frame i
takes record i % D of D distinct records and table i % TABLES of TABLES tables, so a reference is D x TABLES blocks, tiled --
and since D is prime (coprime with 4, 8, 64 and 128) no two neighbouring units, groups or XCD runs hold the same content.
The frames of several units, and one grey frame near the end, have records of their own ("specials").

Nothing here needs a GPU or the library."""
import ctypes as C

import numpy as np

import xcd_grids as xg

D = 251                      # distinct records of the grey frames
TABLES = 3                   # grey frame i takes table (pair) i % TABLES
EDGE_GROUPS = 65535          # the last launch that is permuted: 65535^2 < 2^32 <= 65536^2
BOUNDARY_GROUP = 65408       # 65535 - 65535 % 128: the permuted part of a 65535-group launch ends here
UNITS = {"ON": 262140, "ON_RAGGED": 262138, "OFF": 262146}
GROUPS = {"ON": 65535, "ON_RAGGED": 65535, "OFF": 65537}
BOUNDARY_UNIT = BOUNDARY_GROUP * xg.MIXED_GROUP - 33   # the 4:2:2 frame there: units 261599 .. 261669, groups 65399 .. 65417


def units_of(name):
    return xg.mixed_units([xg.MIXED_SHAPES[name]])


class CountSet:
    """name: a key of UNITS; zero: with the frame that has an empty component (a one-block frame in its place otherwise, as
    xg.MIXED_ORDER_NO_ZERO does) -> n (frames), units, groups, special {frame: shape name} in frame order, unit0 (first unit of
    every frame, and the total behind the last)"""

    def __init__(self, name, zero=True):
        self.name, self.zero, self.units, self.groups = name, zero, UNITS[name], xg.mixed_groups(UNITS[name])
        last = "444"
        at_unit = [(0, "422"), (71, "bw1"), (76, "zero" if zero else "grey1"), (BOUNDARY_UNIT, "422"),
                   (self.units - units_of(last) - 1, "grey1"), (self.units - units_of(last), last)]
        self.special, frame, unit = {}, 0, 0
        for u, shape in at_unit:                      # one-block frames fill the units in between
            assert u >= unit
            frame += u - unit
            self.special[frame] = shape
            frame, unit = frame + 1, u + units_of(shape)
        assert unit == self.units
        self.n = frame
        per = np.ones(self.n, dtype=np.int64)
        for f, shape in self.special.items():
            per[f] = units_of(shape)
        self.unit0 = np.concatenate([[0], np.cumsum(per)])
        self.boundary_frame = [f for f, shape in self.special.items() if self.unit0[f] == BOUNDARY_UNIT][0]
        self.last_grey = sorted(self.special)[-2]

    def planes(self, f):
        return xg.MIXED_SHAPES[self.special.get(f, "grey1")]

    def frames(self):
        """every frame's planes, as xg.mixed_units and xg.mixed_frame_groups take them"""
        return [self.planes(f) for f in range(self.n)]

    def runs(self):
        """the set in frame order as ("grey", first frame, count) and ("special", frame, 1)"""
        out, at = [], 0
        for f in sorted(self.special):
            if f > at:
                out.append(("grey", at, f - at))
            out.append(("special", f, 1))
            at = f + 1
        assert at == self.n                           # (the last frame is a special)
        return out

    def unit_of(self, frame, plane, block):
        """(unit, lane) of a block of a plane of a frame"""
        planes = self.planes(frame)
        assert 0 <= block < planes[plane][0] * planes[plane][1]
        before = sum(-(-bw * bh // xg.MIXED_UNIT) for bw, bh, _ in planes[:plane])
        return int(self.unit0[frame]) + before + block // xg.MIXED_UNIT, block % xg.MIXED_UNIT

    def guard_places(self):
        """(frame, plane, block) of the blocks tests/test_gpu_mixed_counts.py makes fail the int32 guard, all in specials: in the
        first unit (one of them its lane 63), in the last unit of group 65407 (lane 63) and the first of group 65408 (lane 0), the
        only block of the last unit of the boundary frame, the one-block frame before the last frame, and the last block of the set"""
        b = self.boundary_frame
        first = int(self.unit0[b])
        edge = BOUNDARY_GROUP * xg.MIXED_GROUP
        bw, bh, _ = self.planes(b)[2]
        lw, lh, _ = self.planes(self.n - 1)[2]
        return [(0, 0, 5), (0, 0, 63), (b, 0, (edge - 1 - first) * 64 + 63), (b, 0, (edge - first) * 64), (b, 2, bw * bh - 1),
                (self.last_grey, 0, 0), (self.n - 1, 2, lw * lh - 1)]


_SETS = {}


def count_set(name, zero=True):
    if (name, zero) not in _SETS:
        _SETS[name, zero] = CountSet(name, zero)
    return _SETS[name, zero]


def place(s, grey_pitch, special_size, align=1, lead=0):
    """offsets of the frames' records in one buffer: a grey frame's every grey_pitch, a special's of special_size(frame) rounded
    up to align (grey_pitch is a multiple of it) -> (int64 offsets [n], the end of the last record's room)"""
    assert grey_pitch % align == 0 and lead % align == 0
    size = np.full(s.n, grey_pitch, dtype=np.int64)
    for f in s.special:
        size[f] = -(-special_size(f) // align) * align
    ends = lead + np.cumsum(size)
    return np.concatenate([[lead], ends[:-1]]), int(ends[-1])


def fill(s, out, offsets, grey_pitch, grey_rows, special_record):
    """writes every frame's record into out at its offset: grey_rows(frames: int64 array) -> [len][width] rows of the grey
    frames (width <= grey_pitch; what lies between two records keeps what out held), special_record(frame) -> 1-D"""
    for kind, f, k in s.runs():
        at = int(offsets[f])
        if kind == "special":
            rec = special_record(f)
            out[at:at + rec.size] = rec
        else:
            rows = grey_rows(np.arange(f, f + k))
            out[at:at + k * grey_pitch].reshape(k, grey_pitch)[:, :rows.shape[1]] = rows


def size_array(values):
    """int64 numpy array -> a ctypes array of size_t, as the wrappers take it ready"""
    a = np.ascontiguousarray(values, dtype=np.uint64)
    return (C.c_size_t * a.size).from_buffer_copy(a)


def replicate(struct, items, n):
    """a ctypes array (struct * n) whose entry i is a copy of items[i % len(items)]; the bytes are replicated with numpy, no field
    is set from Python per entry -> (the array, its bytes as a numpy view [n][sizeof]: writing a row changes that entry)"""
    raw = np.empty((n, C.sizeof(struct)), dtype=np.uint8)
    for k, item in enumerate(items):
        raw[k::len(items)] = np.frombuffer(bytes(item), dtype=np.uint8)
    return (struct * n).from_buffer(raw), raw         # (the array shares raw's memory and keeps it alive)


def descriptors(struct, s, grey, special):
    """one descriptor per frame of the set s as a ctypes array (struct * n): grey[t] for a grey frame with i % TABLES == t,
    special(frame) for the others"""
    assert len(grey) == TABLES
    arr, raw = replicate(struct, grey, s.n)
    for f in s.special:
        raw[f] = np.frombuffer(bytes(special(f)), dtype=np.uint8)
    return arr


# ---- files for the mixed GPU reader's cap on the table sets of a chunk (csrc/hvc_mixed_reader.h HVC_HDM_MAX_TABLE_SETS) --------
MAX_TABLE_SETS = 512
TABLE_SET_FILES = 520        # grey 16 x 16 files, each with the Huffman tables fitted to its own record
TABLE_SET_SEED = 7000        # seeds 7000 .. 7519 give 520 distinct table sets (tests/test_mixed_counts.py)
REUSERS = (2, 3, 5, 7, 11, 13, 17, 19)   # eight more files with the tables of these, behind file 515
REUSERS_AT = 516


def dht_payload(jpeg):
    """the bodies of the file's DHT segments, in file order: what makes a table set"""
    out, at = [], 2
    while True:
        assert jpeg[at] == 0xFF
        marker, n = jpeg[at + 1], int.from_bytes(jpeg[at + 2:at + 4], "big")
        if marker == 0xC4:
            out.append(jpeg[at + 4:at + 2 + n])
        if marker == 0xDA:
            return b"".join(out)
        at += 2 + n


def table_set_files():
    """-> (files, reusers: their positions).  A re-user is the negated record of its source: the same symbols as often, so
    the same fitted tables, and other bits in the scan"""
    from mixed_reader_files import GREY, grey_file
    from helpers import jpeg_optimised_tables
    from test_restart_intervals import QT, random_record
    files = [grey_file(16, 16, TABLE_SET_SEED + k) for k in range(TABLE_SET_FILES)]
    again = [jpeg_optimised_tables(16, 16, GREY, QT, -np.asarray(random_record(GREY, 16, 16, TABLE_SET_SEED + k)[0]), table_sets=1)
             for k in REUSERS]
    return files[:REUSERS_AT] + again + files[REUSERS_AT:], list(range(REUSERS_AT, REUSERS_AT + len(REUSERS)))


def beyond_the_table_sets(files, cap=MAX_TABLE_SETS):
    """the positions of the files whose table set is not among the first `cap` distinct ones in file order"""
    seen, out = [], []
    for k, f in enumerate(files):
        d = dht_payload(f)
        if d not in seen:
            if len(seen) >= cap:
                out.append(k)
                continue
            seen.append(d)
    return out
