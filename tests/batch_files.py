"""Small file sets the GPU pipeline tests share: raw 4:2:0 frames, files of one geometry, files of mixed geometry."""
from conftest import golden_bytes
from helpers import synth_pixels
from oracle import orc
from test_host_entropy import UNUSUAL_SAMPLINGS, unusual_sampling_file


def frames(n, w, h, seed):
    out = []
    for f in range(n):
        y = synth_pixels(seed + f, h, w)
        u = synth_pixels(seed + 100 + f, h // 2, w // 2)
        v = synth_pixels(seed + 200 + f, h // 2, w // 2)
        out.append((y, u, v))
    return out


def uniform_files(n, seed):
    """n files of one geometry (64 x 64, 4:2:0) and one set of tables, with their raw frames"""
    raw = frames(n, 64, 64, seed)
    return [orc.encode_yuv(y, u, v, 64, 64, 420, 75) for y, u, v in raw], raw


def mixed_files():
    """Mouse480 first (its record alone is a chunk), mini.jpg, unusual samplings at 40 x 24 and 97 x 51"""
    files = [golden_bytes("Mouse480.jpg"), golden_bytes("mini.jpg")]
    files += [unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 40, 24, 100 * si + 40)[0] for si in (0, 3, 9)]
    files += [unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 97, 51, 100 * si + 97)[0] for si in (1, 8)]
    return files
