"""Coefficient records whose SYMBOL HISTOGRAMS have a stated shape, for the tests of the optimised-table coders
(tests/test_huffman_edge_records.py on the CPU, tests/test_gpu_huffman_edges.py on the GPU): Huffman trees deeper than 16
before figure K.3, long runs of equal counts, the whole alphabet, tables of one symbol, a table without EOB.  Natural
frames give none of these.  A record is int16 in the C ABI's layout of hvc_jpeg_encoder_layout(w, h, chroma, q) (`info`
below; only its geometry is read).  symbol_counts is the pure-Python counter the families' properties are asserted with:
nothing here calls the library.

Building blocks: an AC symbol (run, size) is one coefficient of that size behind `run` zeros; ZRL comes from gaps of 16
or more; EOB is one per block that does not end at position 63; DC categories come from the differences between
consecutive blocks of a component in scan order."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from jpeg_opt_writer import _code_sizes, _optimal_lengths  # noqa: E402

EOB, ZRL = 0x00, 0xF0
AC_ALPHABET = [EOB, ZRL] + [(r << 4) | s for r in range(16) for s in range(1, 11)]


# -- geometry -------------------------------------------------------------------------------------------------------

def table_sets(info):
    """[[components of table set 0], [... of set 1]]: set 1 is counted over U and V together"""
    sets = [[], []]
    for i in range(info.n_comp):
        assert info.comp[i].dc_table == info.comp[i].ac_table
        sets[info.comp[i].dc_table].append(i)
    return sets


def mcu_grid(info):
    """(MCUs wide, MCUs high): every plane holds whole MCUs"""
    c, L = info.comp[0], info.layout[0]
    wide, high = L.blocks_w // c.hscale, L.blocks_h // c.vscale
    for i in range(info.n_comp):
        c, L = info.comp[i], info.layout[i]
        assert (L.blocks_w, L.blocks_h) == (wide * c.hscale, high * c.vscale), "planes of whole MCUs only"
    return wide, high


def scan_index(info, ci):
    """the raster block indices of component ci in the order the scan codes them"""
    wide, high = mcu_grid(info)
    c, bw = info.comp[ci], info.layout[ci].blocks_w
    return np.array([(my * c.vscale + sy) * bw + mx * c.hscale + sx for my in range(high) for mx in range(wide)
                     for sy in range(c.vscale) for sx in range(c.hscale)])


def blocks_of(info, rec, ci):
    """view [n][64] of component ci's blocks (plane raster order) inside a record"""
    L = info.layout[ci]
    n = L.blocks_w * L.blocks_h
    return rec[L.coef_offset:L.coef_offset + n * 64].reshape(n, 64)


def n_blocks(info, comps):
    return sum(info.layout[i].blocks_w * info.layout[i].blocks_h for i in comps)


# -- the counter ----------------------------------------------------------------------------------------------------

def _cat(v):
    return int(abs(int(v))).bit_length()


def ac_symbols(block):
    """the AC symbols of one block [64], in order"""
    out, prev = [], 0
    for k in np.flatnonzero(block[1:]) + 1:
        run = int(k) - prev - 1
        prev = int(k)
        out += [ZRL] * (run >> 4)
        out.append(((run & 15) << 4) | _cat(block[k]))
    if prev != 63:
        out.append(EOB)
    return out


def symbol_counts(info, rec, restart_interval=0):
    """[DC0, DC1, AC0, AC1]: 256 counts each, over the scan of one record; restart_interval: the DC predictors start
    again at zero every so many MCUs"""
    counts = [[0] * 256 for _ in range(4)]
    wide, high = mcu_grid(info)
    blocks = [blocks_of(info, rec, i) for i in range(info.n_comp)]
    pred = [0] * info.n_comp
    for m in range(wide * high):
        my, mx = divmod(m, wide)
        if restart_interval and m % restart_interval == 0:
            pred = [0] * info.n_comp
        for ci in range(info.n_comp):
            c, bw, t = info.comp[ci], info.layout[ci].blocks_w, info.comp[ci].dc_table
            for sy in range(c.vscale):
                for sx in range(c.hscale):
                    b = blocks[ci][(my * c.vscale + sy) * bw + mx * c.hscale + sx]
                    counts[t][_cat(int(b[0]) - pred[ci])] += 1
                    pred[ci] = int(b[0])
                    for s in ac_symbols(b):
                        counts[2 + t][s] += 1
    return counts


def max_code_size(freq):
    """the largest code size before figure K.3 among the coded symbols"""
    return max(_code_sizes(freq)[:256])


def code_lengths(freq):
    """{symbol: code length after figure K.3}"""
    bits, vals = _optimal_lengths(freq)
    out, k = {}, 0
    for ln in range(1, 17):
        for _ in range(bits[ln]):
            out[vals[k]] = ln
            k += 1
    return out


# -- AC: blocks from counts -------------------------------------------------------------------------------------------

def _value(size, k):
    """some coefficient of that size, varying with k"""
    mag = (1 << (size - 1)) + (k * 7 + size) % (1 << (size - 1))
    return mag if k & 1 else -mag


def pack_ac(counts, n):
    """n blocks [n][64] (DC zero) whose AC symbols have EXACTLY these counts ({symbol: count}, EOB and ZRL included):
    n - counts[EOB] blocks are filled to position 63, the others end before it.  Every ZRL goes in front of a coefficient
    of its own (the cheapest symbols first).  Greedy, largest item first; raises where it does not come out.  The blocks
    come back in a seeded random order, so that every component and every tile of a table set gets its share."""
    counts = {s: int(c) for s, c in counts.items() if c}
    assert all(s in AC_ALPHABET for s in counts), "a symbol outside the baseline alphabet"
    n_eob, n_zrl = counts.get(EOB, 0), counts.get(ZRL, 0)
    n_full = n - n_eob
    assert 0 <= n_full, "more EOBs than blocks"
    # items [length in positions, symbol]; a ZRL lengthens an item by 16: dealt in turn, the cheapest symbols first
    syms = sorted((s for s in counts if s not in (EOB, ZRL)), key=lambda s: (s >> 4, -counts[s], s))
    items = [[(s >> 4) + 1, s] for s in syms for _ in range(counts[s])]
    for z in range(n_zrl):
        it = items[z % len(items)]
        assert it[0] + 16 <= 63, "a ZRL too many"
        it[0] += 16
    by_len = {}
    for it in items:
        by_len.setdefault(it[0], []).append(it)
    blk = np.zeros((n, 64), dtype=np.int16)
    serial = 0

    def fill(b, room_max, exact):
        nonlocal serial
        pos = 0
        while pos < room_max:
            fits = [ln for ln in by_len if ln <= room_max - pos]
            if not fits:
                break
            ln = max(fits)                 # the largest item that fits: the single positions stay for the last gaps
            ln, s = by_len[ln].pop()
            if not by_len[ln]:
                del by_len[ln]
            pos += ln
            blk[b, pos] = _value(s & 15, serial)
            serial += 1
        assert not exact or pos == room_max, "block %d cannot be filled to position 63" % b
        return pos

    for b in range(n_full):
        fill(b, 63, True)
    for b in range(n_full, n):
        fill(b, 62, False)
    assert not by_len, "%d coefficients left over" % sum(len(v) for v in by_len.values())
    return blk[np.random.default_rng(n).permutation(n)]


def put_ac(info, rec, comps, blk):
    """deal the blocks' AC coefficients [n][64] to the components of one table set, in turn"""
    at = 0
    for ci in comps:
        dst = blocks_of(info, rec, ci)
        dst[:, 1:] = blk[at:at + len(dst), 1:]
        at += len(dst)
    assert at == len(blk)


# -- DC ---------------------------------------------------------------------------------------------------------------

def put_dc_categories(info, rec, ci, cats):
    """component ci's DC values such that the j-th block of its scan has a difference of category cats[j % len(cats)] to
    the one before; the signs keep the values small"""
    order = scan_index(info, ci)
    dc, vals = 0, []
    for j in range(len(order)):
        k = cats[j % len(cats)]
        d = 0 if k == 0 else (1 << (k - 1)) + (j % (1 << (k - 1)))
        dc += d if dc <= 0 else -d
        vals.append(dc)
    blocks_of(info, rec, ci)[order, 0] = np.array(vals, dtype=np.int16)


def sparse_random(info, seed, density=0.15, cmax=60, dcmax=200):
    """an ordinary record: seeded sparse random coefficients"""
    rng = np.random.default_rng(seed)
    rec = np.zeros(info.coef_count, dtype=np.int16)
    for ci in range(info.n_comp):
        b = blocks_of(info, rec, ci)
        c = rng.integers(-cmax, cmax + 1, size=b.shape)
        c *= rng.random(size=b.shape) < density
        c[:, 0] = rng.integers(-dcmax, dcmax + 1, size=len(b))
        b[:] = c
    return rec


# -- the families -----------------------------------------------------------------------------------------------------

def chain_counts(n_sym, eob):
    """n_sym counts in ascending order, `eob` one of them (-> its index), that merge as ONE CHAIN under Annex K.2: with
    the reserved symbol's 1 in front, every count is larger than the sum of all but the one before it, so the two smallest
    nodes are always the merged one and the next count.  Without `eob` forced in: 1, 2, 3, 5, 8 ... (Fibonacci), the
    cheapest such chain.  Code sizes before figure K.3: n_sym for the rarest (and the reserved symbol), one less for each
    count after."""
    a, total, at = [], 1, None          # total = the reserved symbol + the counts so far
    while len(a) < n_sym:
        lo = 1 if not a else max(a[-1], total - a[-1] + 1)
        if at is None and eob is not None and (eob < max(lo, total + 1) or len(a) == n_sym - 1):
            assert eob >= lo
            at = len(a)
            a.append(eob)
        else:
            a.append(lo)
        total += a[-1]
    return a, at


def _chain_symbols(n):
    """n AC symbols, rarest first: the two rarest have size 10 (a 16-bit code then carries 10 value bits); towards the
    frequent end the symbols get cheap (run 0)"""
    rare = [0x0A, 0x1A]
    rest = sorted((s for s in AC_ALPHABET if s not in (EOB, ZRL, 0x0A, 0x1A)), key=lambda s: (s >> 4, s & 15))
    return rare + rest[:n - 2][::-1]


def chain_ac_counts(depth, n):
    """{symbol: count} of a chain `depth` symbols long that fits n blocks exactly: the EOB count is whatever the blocks
    that do not end at position 63 come to, so it is searched for -- the smallest one for which the other counts' coefficients
    fill n - eob blocks to position 63 and leave no more than the eob blocks can hold"""
    syms = _chain_symbols(depth - 1)
    for eob in range(1, n + 1):
        a, at = chain_counts(depth, eob)
        others = a[:at] + a[at + 1:]
        need = sum(c * ((s >> 4) + 1) for s, c in zip(syms, others))
        if 63 * (n - eob) <= need <= 63 * (n - eob) + 56 * eob:
            out = dict(zip(syms, others))
            out[EOB] = eob
            return out
    raise AssertionError("no chain of %d symbols fits %d blocks" % (depth, n))


def chain(info, depth, dc_cats=(0, 1, 2, 3, 2, 1, 4, 0, 5)):
    """both AC tables: one chain of `depth` symbols, code sizes up to `depth` before figure K.3"""
    rec = np.zeros(info.coef_count, dtype=np.int16)
    for comps in table_sets(info):
        n = n_blocks(info, comps)
        put_ac(info, rec, comps, pack_ac(chain_ac_counts(depth, n), n))
        for ci in comps:
            put_dc_categories(info, rec, ci, list(dc_cats))
    return rec


def chain17(info):
    return chain(info, 17)


def chain20(info):
    return chain(info, 20)


def ties(info):
    """AC: every symbol but EOB exactly once per table set; DC: the twelve categories in turn (equal counts where the
    component's block count is a multiple of 12)"""
    rec = np.zeros(info.coef_count, dtype=np.int16)
    for comps in table_sets(info):
        n = n_blocks(info, comps)
        counts = {s: 1 for s in AC_ALPHABET}
        counts[EOB] = n - 4                        # four blocks filled to position 63, all others end early
        put_ac(info, rec, comps, pack_ac(counts, n))
        for ci in comps:
            put_dc_categories(info, rec, ci, list(range(12)))
    return rec


def whole_alphabet_counts(n):
    """{symbol: count} for n blocks: every symbol present, EOB in every block, and as many pairwise different counts as
    the blocks hold -- the m cheapest symbols get m + 1 ... 2 (run 0 the most), the others 1"""
    syms = sorted((s for s in AC_ALPHABET if s != EOB), key=lambda s: (16 if s == ZRL else s >> 4, s & 15))
    cost = lambda s: 17 if s == ZRL else (s >> 4) + 1
    best = None
    for m in range(len(syms) + 1):
        counts = {s: (m + 1 - i if i < m else 1) for i, s in enumerate(syms)}
        if sum(c * cost(s) for s, c in counts.items()) > 56 * n:   # 62 positions a block, less what greedy packing wastes
            break
        best = counts
    assert best is not None, "%d blocks do not hold the alphabet" % n
    best[EOB] = n
    return best


def whole_alphabet(info):
    """helpers.every_symbol_record (its DC: the twelve categories in turn), with AC counts that differ from symbol to
    symbol as far as the blocks allow"""
    from helpers import every_symbol_record
    rec = every_symbol_record(info)
    for comps in table_sets(info):
        n = n_blocks(info, comps)
        put_ac(info, rec, comps, pack_ac(whole_alphabet_counts(n), n))
    return rec


def eob_only(info):
    """every AC table holds EOB alone, every DC table category 0 alone"""
    return np.zeros(info.coef_count, dtype=np.int16)


def no_eob(info, seed=11):
    """chroma: every block ends at position 63, so table set 1 never codes an EOB; luma: ordinary"""
    rec = sparse_random(info, seed)
    for ci in table_sets(info)[1]:
        b = blocks_of(info, rec, ci)
        b[:, 63] = np.where(np.arange(len(b)) & 1, 3, -1)
    return rec


def one_dc_category(info, d=37, seed=12):
    """DC differences all of one non-zero category: the values alternate between d and 0 along every component's scan"""
    rec = sparse_random(info, seed)
    for ci in range(info.n_comp):
        order = scan_index(info, ci)
        blocks_of(info, rec, ci)[order, 0] = np.where(np.arange(len(order)) & 1, 0, d).astype(np.int16)
    return rec


# name -> (builder, [(w, h, chroma)] the family's own geometries)
FAMILIES = {
    "chain17": (chain17, [(128, 128, 444)]),
    "chain20": (chain20, [(256, 192, 444), (512, 256, 420)]),
    "ties": (ties, [(128, 96, 444)]),
    "whole_alphabet": (whole_alphabet, [(128, 88, 444)]),
    "eob_only": (eob_only, [(64, 48, 420)]),
    "no_eob": (no_eob, [(64, 48, 420)]),
    "one_dc_category": (one_dc_category, [(64, 48, 444)]),
}
CASES = [(name, w, h, chroma) for name, (_, geoms) in FAMILIES.items() for (w, h, chroma) in geoms]
QUALITY = 75


def check_property(name, info, rec):
    """the family's stated property, from the Python counter alone; returns the counts"""
    dc0, dc1, ac0, ac1 = counts = symbol_counts(info, rec)
    present = lambda c: [s for s in range(256) if c[s]]
    if name == "chain17":
        assert max(info.layout[i].blocks_w * info.layout[i].blocks_h for i in range(3)) <= 512
        assert max_code_size(ac0) >= 17
    elif name == "chain20":
        assert max(info.layout[i].blocks_w * info.layout[i].blocks_h for i in range(3)) <= 2048
        for ac in (ac0, ac1):
            assert max_code_size(ac) >= 20
            lengths = code_lengths(ac)
            assert max(lengths.values()) == 16
            assert any(ln == 16 and (s & 15) == 10 and ac[s] for s, ln in lengths.items()), "no 26-bit emission"
    elif name == "ties":
        assert min(info.layout[i].blocks_w * info.layout[i].blocks_h for i in range(3)) >= 176
        for ac in (ac0, ac1):
            assert sum(1 for s in present(ac) if ac[s] == min(ac[s] for s in present(ac))) >= 100
        for dc in (dc0, dc1):
            assert present(dc) == list(range(12)) and len(set(dc[:12])) == 1
    elif name == "whole_alphabet":
        for ac, distinct in ((ac0, 60), (ac1, 90)):
            assert present(ac) == sorted(AC_ALPHABET)
            # 176 / 352 blocks of 62 positions hold about 70 / 100 different counts when the cheap symbols take the large ones
            assert len(set(ac[s] for s in AC_ALPHABET)) >= distinct
        for dc in (dc0, dc1):
            assert present(dc) == list(range(12))
    elif name == "eob_only":
        assert present(ac0) == present(ac1) == [EOB] and present(dc0) == present(dc1) == [0]
    elif name == "no_eob":
        assert ac1[EOB] == 0 and ac0[EOB] > 0 and len(present(ac1)) > 4 and len(present(ac0)) > 4
    elif name == "one_dc_category":
        assert present(dc0) == present(dc1) and len(present(dc0)) == 1 and present(dc0)[0] > 0
        assert len(present(ac0)) > 4 and len(present(ac1)) > 4
    else:
        raise KeyError(name)
    return counts
