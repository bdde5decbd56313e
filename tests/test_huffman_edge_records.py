"""The record families of tests/huffman_records.py on the host: every family has the property it is named for (from the
pure-Python counter), and the host coder (csrc/hvc_entropy.cpp: hvc_huffman_optimal_tables, hvc_jpeg_entropy_encode_tables
and their restart twins) agrees byte for byte with the Annex K.2 writer of tools/jpeg_opt_writer.py on them -- trees that
figure K.3 has to shorten, 16-bit codes with 10 value bits behind them, tables of a single symbol, a table without EOB.
Host C++ only.  tests/test_gpu_huffman_edges.py holds the GPU table builder to the same writer."""
import numpy as np
import pytest

import huffman_records as R
from jpeg_opt_writer import _code_sizes, _optimal_lengths, jpeg_optimised_tables
from test_huffman_optimise import segments, writer_accepts

# (family, w, h, chroma, restart interval)
CASES = [c + (0,) for c in R.CASES] + [c + (ri,) for c in R.CASES if c[0] in ("chain20", "eob_only") for ri in (1, 5)]


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    m.build()
    return m.hvc


@pytest.mark.parametrize("name,w,h,chroma,ri", CASES, ids=["%s-%dx%d-%d-ri%d" % c for c in CASES])
def test_family_on_the_host(hvc, name, w, h, chroma, ri):
    info = hvc.jpeg_encoder_layout(w, h, chroma, R.QUALITY)
    assert writer_accepts(info, w, h, chroma)
    rec = R.FAMILIES[name][0](info)
    assert rec.dtype == np.int16 and rec.size == info.coef_count
    R.check_property(name, info, rec)
    # the tables: Annex K.2 over the Python counter's counts (of the scan cut every ri MCUs)
    counts = R.symbol_counts(info, rec, ri)
    want_specs = []
    for c in counts:
        bits, vals = _optimal_lengths(c)
        want_specs.append((bits[1:17], vals))
    assert hvc.huffman_optimal_tables(info, rec, ri) == want_specs
    # the file: DHT bodies and entropy-coded segment
    jpg = hvc.jpeg_entropy_encode(info, rec, "optimised", restart_interval=ri)
    want = jpeg_optimised_tables(w, h, chroma, info.qtab_array(), rec, table_sets=2, restart_interval=ri)
    dht, ecs = segments(jpg)
    wdht, wecs = segments(want)
    assert dht == wdht
    assert ecs == wecs
    for t, (bits, vals) in enumerate(want_specs):
        assert dht[(t >> 1, t & 1)] == bytes(bits) + bytes(vals)
    # ... and back
    _, got = hvc.jpeg_entropy_decode(jpg, restart_markers=bool(ri))
    assert np.array_equal(got.reshape(-1)[:rec.size], rec)


def test_code_sizes_split_keeps_optimal_lengths():
    """_code_sizes is _optimal_lengths' first half: a Fibonacci chain of 30 counts has sizes up to 30 before figure K.3 and
    16 after, and the symbols leave in (size, symbol) order"""
    fib = [1, 2]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    freq = [0] * 256
    for i, f in enumerate(fib):
        freq[i * 7] = f
    sizes = _code_sizes(freq)
    assert len(sizes) == 257 and max(sizes[:256]) == 30 and sizes[256] == 30
    assert [s for s in range(256) if sizes[s]] == [i * 7 for i in range(30)]
    bits, vals = _optimal_lengths(freq)
    assert sum(bits) == len(vals) == 30 and max(l for l in range(17) if bits[l]) == 16
    assert vals == sorted(vals, key=lambda s: (sizes[s], s))


def test_chain_counts_are_one_chain():
    """the chain builder with an EOB count forced in at the rare end, in the middle, and above every other count"""
    for n_sym, eob in ((17, None), (20, 1), (20, 300), (20, 5000), (12, 10 ** 6)):
        a, at = R.chain_counts(n_sym, eob)
        assert a == sorted(a) and len(a) == n_sym and (eob is None or a[at] == eob)
        freq = [0] * 256
        for i, c in enumerate(a):
            freq[i] = c
        sizes = _code_sizes(freq)
        assert sizes[256] == n_sym and sizes[:n_sym] == list(range(n_sym, 0, -1))


def test_unused_table_set_is_invalid_arg(hvc):
    """all components on one table set: the other has no symbol to fit a table to (the GPU entry points answer the same)"""
    import ctypes as C
    info = hvc.jpeg_encoder_layout(64, 48, 444, R.QUALITY)
    rec = R.sparse_random(info, 3)
    for sel in (0, 1):
        one = hvc.JpegInfo.from_buffer_copy(info)
        for i in range(3):
            one.comp[i].dc_table = one.comp[i].ac_table = sel
        assert hvc.lib().hvc_jpeg_encoder_check(C.byref(one)) == 0
        out = (hvc.HuffSpec * 4)()
        assert hvc.lib().hvc_huffman_optimal_tables(C.byref(one), rec.ctypes.data, out) == -1
        assert hvc.lib().hvc_huffman_optimal_tables_restart(C.byref(one), rec.ctypes.data, 2, out) == -1
