"""Files and records for the libjpeg-exact decoder's tests (tests/test_libjpeg_reference.py on the CPU,
tests/test_gpu_libjpeg.py on the GPU, tests/golden/make_libjpeg_pins.py): written by tools/jpeg_opt_writer.py from seeded
random coefficient records, so that a case is named by its parameters and nothing but the two golden files is stored."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from jpeg_opt_writer import jpeg_optimised_tables  # noqa: E402

# sampling -> the components' (h, v) factors as the writer takes them
FACTORS = {420: [(2, 2), (1, 1), (1, 1)], 422: [(2, 1), (1, 1), (1, 1)], 444: [(1, 1)] * 3, 400: [(1, 1)]}
SIZES = [(1, 1), (3, 2), (4, 4), (5, 5), (6, 3), (16, 16), (17, 9), (18, 10), (33, 31), (53, 45), (64, 48)]
# (density, |c| <=, q <=): sparse ordinary, half-dense, rare large coefficients
FAMILIES = [(0.15, 60, 12), (0.5, 25, 30), (0.05, 1023, 3)]
# what libjpeg-turbo's SIMD does NOT reproduce of the definition (16-bit wrap): dense blocks under large table entries --
# never held against Pillow
DENSE = (1.0, 8, 255)
DENSE_Q64 = (1.0, 8, 64)   # agreed with Pillow where it was tried


def planes_of(w, h, sampling):
    """[(blocks_w, blocks_h, table index)] of the decoder's padded planes (decoder.ml:294-345)"""
    f = FACTORS[sampling]
    hs, vs = max(a for a, _ in f), max(b for _, b in f)
    up = lambda x, m: (x + m - 1) // m * m
    wr, hr = up(w, 8 * hs), up(h, 8 * vs)
    return [(wr * a // hs // 8, hr * b // vs // 8, 0 if i == 0 else 1) for i, (a, b) in enumerate(f)]


def random_record(seed, w, h, sampling, family):
    """(tables [2][64] uint16, the frame's coefficient record int16, planes): |DC * q| <= 1000"""
    density, cmax, qmax = family
    rng = np.random.default_rng(seed)
    planes = planes_of(w, h, sampling)
    q = rng.integers(1, qmax + 1, size=(2, 64)).astype(np.uint16)
    parts = []
    for bw, bh, t in planes:
        c = rng.integers(-cmax, cmax + 1, size=(bh * bw, 64))
        c *= rng.random(size=c.shape) < density
        lim = 1000 // int(q[t, 0])
        c[:, 0] = rng.integers(-lim, lim + 1, size=bh * bw)
        parts.append(c.reshape(-1))
    return q, np.concatenate(parts).astype(np.int16), planes


def writer_file(seed, w, h, sampling, family, restart_interval=0):
    """(jpeg bytes, tables, record, planes)"""
    q, c, planes = random_record(seed, w, h, sampling, family)
    return jpeg_optimised_tables(w, h, FACTORS[sampling], q, c, restart_interval=restart_interval), q, c, planes


def seed_of(w, h, sampling, fam):
    return 7000 + 1000 * fam + 97 * w + 13 * h + sampling


# the writer-made files whose Pillow RGB is pinned in tests/golden/libjpeg_pins.json: (w, h, sampling, family index, restart interval)
PINNED = [(53, 45, 420, 0, 0), (17, 9, 422, 1, 0), (33, 31, 444, 2, 0), (18, 10, 400, 0, 0), (4, 4, 420, 1, 0), (64, 48, 420, 0, 3),
          (5, 5, 422, 2, 0)]
GOLDEN_FILES = ["Mouse480.jpg", "mini.jpg"]


def pin_name(w, h, sampling, fam, ri):
    return "writer_%dx%d_%d_family%d_seed%d%s" % (w, h, sampling, fam, seed_of(w, h, sampling, fam), "_ri%d" % ri if ri else "")


def pinned_file(case):
    w, h, sampling, fam, ri = case
    return writer_file(seed_of(w, h, sampling, fam), w, h, sampling, FAMILIES[fam], ri)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint8).tobytes()).hexdigest()


def sampling_of_info(info):
    if info.n_comp == 1:
        return 400
    return {(2, 2): 420, (2, 1): 422, (1, 1): 444}[(info.comp[0].hscale, info.comp[0].vscale)]


def planes_of_info(info):
    return [(info.layout[k].blocks_w, info.layout[k].blocks_h, info.layout[k].qtab) for k in range(info.n_comp)]
