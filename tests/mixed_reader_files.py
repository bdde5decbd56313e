"""The file set of the mixed GPU Huffman reader's tests (tests/test_gpu_mixed_reader.py, tests/test_hdec_mixed_plan.py): built
once per process from the suite's own generators, seeds fixed."""
import functools

import numpy as np

from conftest import golden_bytes
from helpers import jpeg_optimised_tables
from test_host_entropy import UNUSUAL_SAMPLINGS, unusual_sampling_file
from test_restart_intervals import QT, random_record

SUBSEQ_BYTES = 128
GREY = [(1, 1)]


def segment_bytes(jpeg):
    """length of the file's unstuffed entropy-coded segment: what stands between the SOS header and the marker behind the scan"""
    at = jpeg.index(b"\xff\xda")
    at += 2 + int.from_bytes(jpeg[at + 2:at + 4], "big")
    n = 0
    while True:
        b = jpeg[at]
        if b == 0xFF:
            if jpeg[at + 1] != 0:
                return n
            at += 1
        n += 1
        at += 1


def subsequences(jpeg):
    return -(-segment_bytes(jpeg) // SUBSEQ_BYTES) + 1


def grey_file(w, h, seed):
    return jpeg_optimised_tables(w, h, GREY, QT, random_record(GREY, w, h, seed)[0], table_sets=1)


def dense_file(w, h, seed):
    """every coefficient nonzero, magnitudes up to 1023, under the model's default tables: a block is 63 codes of up to 16 bits
    with up to ten magnitude bits each -- around 200 bytes, so every block spans three 128-byte subsequences or more"""
    import video_coding_amd as m
    info = m.hvc.jpeg_encoder_layout(w, h, 420, 50)
    rng = np.random.Generator(np.random.PCG64(seed))
    blocks = (rng.integers(1, 1024, size=(info.coef_count // 64, 64)) * rng.choice([-1, 1], size=(info.coef_count // 64, 64))).astype(np.int16)
    blocks[:, 0] = rng.integers(-900, 901, size=blocks.shape[0])   # (DC differences within the categories the default tables code)
    return m.hvc.jpeg_entropy_encode(info, blocks.reshape(-1))


def flat_grey_file(w, h, dc=37):
    """constant DC, no AC: every block after the first is the same two short codes -- the bit pattern is periodic, and a walk
    that starts out of step never falls into step"""
    n = (-(-w // 8)) * (-(-h // 8))
    rec = np.zeros((n, 64), dtype=np.int16)
    rec[:, 0] = dc
    return jpeg_optimised_tables(w, h, GREY, QT, rec.reshape(-1), table_sets=1)


@functools.lru_cache(maxsize=None)
def reader_set():
    """-> (files, names, ineligible): the file set of tests/test_gpu_mixed.py and the reader's own corner cases; ineligible =
    the indices the GPU reader cannot take (21 blocks per MCU, four components)"""
    from test_gpu_hdec import _many_prefix_file
    files, names = [golden_bytes("mini.jpg"), golden_bytes("Mouse480.jpg")], ["mini", "mouse480"]
    for si in (0, 1, 3, 4, 6, 8, 9, 10, 11):
        files.append(unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 40, 24, 100 * si + 40)[0])
        names.append("sampling%d-40x24" % si)
    for si in (2, 5, 7, 8, 10):
        files.append(unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 97, 51, 100 * si + 97)[0])
        names.append("sampling%d-97x51" % si)
    for seed in (1, 2):   # one geometry, different optimised Huffman tables
        files.append(jpeg_optimised_tables(96, 64, 420, QT, random_record([(2, 2), (1, 1), (1, 1)], 96, 64, seed)[0]))
        names.append("optimised-seed%d" % seed)
    ineligible = [i for i, n in enumerate(names) if n.startswith("sampling8-") or n.startswith("sampling11-")]
    files.append(grey_file(8, 8, 5))                       # one block, one subsequence (and the zero one behind it)
    names.append("grey-8x8")
    # (the seeds below: the first of a search over grey_file's seeds, 0 upwards, that gives the length wanted)
    for residue, seed in ((127, 34), (0, 18), (1, 2089)):  # the segment ends one byte before a subsequence boundary, at it, one past
        f = grey_file(32, 32, seed)
        assert segment_bytes(f) % SUBSEQ_BYTES == residue
        files.append(f)
        names.append("tiny-mod%d" % residue)
    for subs, seed in ((64, 1), (65, 53)):                 # a unit boundary
        f = grey_file(224, 176, seed)
        assert subsequences(f) == subs
        files.append(f)
        names.append("subs%d" % subs)
    big = jpeg_optimised_tables(640, 416, 420, QT, random_record([(2, 2), (1, 1), (1, 1)], 640, 416, 77)[0])
    assert subsequences(big) > 512
    files.append(big)
    names.append("subs-over-512")
    files.append(dense_file(24, 16, 9))
    names.append("dense")
    files.append(_many_prefix_file(2100, 130, 70, 422, 60)[0])
    names.append("overflow-prefixes")
    return files, names, ineligible
