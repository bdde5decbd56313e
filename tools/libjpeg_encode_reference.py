"""The encoder of include/hvc_jpeg.h ("Encoding bit-exact to libjpeg": hvc_set_encode_libjpeg) in numpy int64: the checker
of k_fdct_islow, k_dummy_blocks and k_rgb_to_ycc_libjpeg.  Pure numpy, no library of the project: what it computes is held
against libjpeg-turbo (through PIL) by tests/test_libjpeg_encode_reference.py, and the GPU against it by
tests/test_gpu_libjpeg_encode.py.

    block stage   libjpeg's jfdctint.c ("islow") on p - 128: the operation list of csrc/hvc_fdct_islow_spec.h, parsed from
                  that file and replayed here; then sign(t) * ((|t| + 4 q) // (8 q)), stored at the zig-zag position
    edges         every component replicated to the right and downward; blocks past ceil(actual / 8) in either direction are
                  dummy blocks: AC 0, DC of the block before them in the MCU's buffer order (jccoefct.c compress_data)
    from RGB      the colour step of tools/rgb_reference.py, then jcsample.c's h2v2 / h2v1 averaging with alternating bias

Records are in the C ABI's layout: component planes back to back, [blocks_h][blocks_w][64] int16 in zig-zag order with the
DC absolute; tables are 64 entries in zig-zag order."""
import os
import re

import numpy as np

# natural position (8 * row + col) -> zig-zag position
ZF = np.array([0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40,
               44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36,
               48, 49, 57, 58, 62, 63])

# sampling -> the components' (h, v) factors
FACTORS = {420: [(2, 2), (1, 1), (1, 1)], 422: [(2, 1), (1, 1), (1, 1)], 444: [(1, 1)] * 3, 400: [(1, 1)]}

SPEC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-coding_amd", "csrc",
                    "hvc_fdct_islow_spec.h")


# ---- the spec file
def spec_constants():
    """the plain-integer #define's of hvc_fdct_islow_spec.h as {name: int}"""
    return {name: int(val) for name, val in re.findall(r"^#define\s+(HVC_FI_\w+)\s+(\d+)u?\s*$", open(SPEC).read(), flags=re.M)}


def spec_step():
    """the operation list HVC_FDCT_ISLOW_STEP as [(op, args...)]: ("MUL", d, a, k) with k an int, ("ADD" | "SUB", d, a, b),
    ("OUTLO" | "OUTHI", i, a)"""
    text, k = open(SPEC).read(), spec_constants()
    body = text[text.index("#define HVC_FDCT_ISLOW_STEP("):]
    body = body[body.index(")") + 1:body.index("#endif")].replace("\\\n", " ")
    ops = []
    for op, args in re.findall(r"\b(MUL|ADD|SUB|OUTLO|OUTHI)\(([^)]*)\)", body):
        a = [x.strip() for x in args.split(",")]
        if op == "MUL":
            sign, name = (-1, a[2][1:]) if a[2].startswith("-") else (1, a[2])
            ops.append((op, a[0], a[1], sign * k[name]))
        elif op in ("ADD", "SUB"):
            ops.append((op, a[0], a[1], a[2]))
        else:
            ops.append((op, int(a[0]), a[1]))
    assert sorted(o[1] for o in ops if o[0] in ("OUTLO", "OUTHI")) == list(range(8)), "the step has eight results"
    return ops


def replay_step(v, mul, add, sub, ops=None):
    """The step on v[0..7] over any value type: mul(a, k), add(a, b), sub(a, b) -> {i: ("OUTLO" | "OUTHI", value)}.  visit order
    is the list's; every intermediate value is returned under its name as well (key = str)."""
    env = {"v%d" % i: v[i] for i in range(8)}
    out = {}
    for o in ops or spec_step():
        if o[0] == "MUL":
            env[o[1]] = mul(env[o[2]], o[3])
        elif o[0] == "ADD":
            env[o[1]] = add(env[o[2]], env[o[3]])
        elif o[0] == "SUB":
            env[o[1]] = sub(env[o[2]], env[o[3]])
        else:
            out[o[1]] = (o[0], env[o[2]])
    out.update(env)
    return out


def D(x, n):
    return (x + (1 << (n - 1))) >> n


# ---- block stage
def fdct_islow(samples):
    """[..., 8, 8] uint8 samples -> t[..., 8, 8] int64, the DCT scaled by 8 (natural order)"""
    k, ops = spec_constants(), spec_step()
    x = np.asarray(samples).astype(np.int64) - k["HVC_FI_LEVEL"]
    mul, add, sub = (lambda a, c: a * c), (lambda a, b: a + b), (lambda a, b: a - b)
    rows = []  # pass 1: along the rows
    for r in range(8):
        o = replay_step([x[..., r, c] for c in range(8)], mul, add, sub, ops)
        rows.append([o[i][1] << k["HVC_FI_PASS1_LO_SHL"] if o[i][0] == "OUTLO" else D(o[i][1], k["HVC_FI_PASS1_HI_SHIFT"])
                     for i in range(8)])
    cols = []  # pass 2: down the columns
    for c in range(8):
        o = replay_step([rows[r][c] for r in range(8)], mul, add, sub, ops)
        cols.append([D(o[i][1], k["HVC_FI_PASS2_LO_SHIFT"] if o[i][0] == "OUTLO" else k["HVC_FI_PASS2_HI_SHIFT"])
                     for i in range(8)])
    return np.stack([np.stack([cols[c][r] for c in range(8)], axis=-1) for r in range(8)], axis=-2)


def quantise(t, qtab):
    """t[..., 8, 8] (natural order), a zig-zag table of 64 entries in 1..255 -> [..., 64] int16 in zig-zag order"""
    q = np.asarray(qtab).astype(np.int64).reshape(64)
    assert q.min() >= 1 and q.max() <= 255
    t = np.asarray(t).astype(np.int64).reshape(t.shape[:-2] + (64,))
    d = 8 * q[ZF]  # the divisor of natural position k
    v = np.sign(t) * ((np.abs(t) + d // 2) // d)
    out = np.empty_like(v)
    out[..., ZF] = v
    return out.astype(np.int16)


def fdct_quant_plane(plane, qtab):
    """a plane of bh * 8 x bw * 8 samples, every block real -> [bh * bw, 64]"""
    p = np.asarray(plane)
    bh, bw = p.shape[0] // 8, p.shape[1] // 8
    assert p.shape == (bh * 8, bw * 8)
    blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    return quantise(fdct_islow(blocks), qtab).reshape(bh * bw, 64)


# ---- edges
def replicate(plane, pw, ph):
    """aw x ah -> pw x ph, the last column and the last row repeated"""
    p = np.asarray(plane)
    return np.pad(p, ((0, ph - p.shape[0]), (0, pw - p.shape[1])), mode="edge")


def dummy_source(bx, by, real_w, real_h, h, v):
    """The block whose DC a block of a component with sampling factors h x v takes: itself when it is real.  A dummy past the
    real columns in a real row takes the block to its left; a block of a dummy row takes the last block of the row above
    inside its MCU (and so on through dummies)."""
    while True:
        if by >= real_h:
            bx, by = bx // h * h + h - 1, by - 1
            assert by // v == (by + 1) // v, "a dummy row is never an MCU's first"
        elif bx >= real_w:
            assert bx % h, "a dummy column is never an MCU's first"
            bx -= 1
        else:
            return bx, by


def apply_dummies(rec, bw, bh, real_w, real_h, h, v):
    """[bh * bw, 64] with every block computed -> the dummy rule applied in place"""
    rec = rec.reshape(bh, bw, 64)
    for by in range(bh):
        for bx in range(bw):
            sx, sy = dummy_source(bx, by, real_w, real_h, h, v)
            if (sx, sy) != (bx, by):
                rec[by, bx, :] = 0
                rec[by, bx, 0] = rec[sy, sx, 0]
    return rec.reshape(bh * bw, 64)


def geometry(width, height, sampling, factors=None):
    """[(blocks_w, blocks_h, h, v)] per component: whole MCUs, as the file's layout (hvc_jpeg_info.layout) has them.
    factors: the components' (h, v) where they are not libjpeg's for the sampling -- this library's 4:2:2 files are the
    model's (2, 2), (1, 2), (1, 2), whose MCU is 16 rows high: the same planes, a dummy row more where the height asks"""
    f = factors or FACTORS[sampling]
    hs, vs = max(a for a, _ in f), max(b for _, b in f)
    mw, mh = -(-width // (8 * hs)), -(-height // (8 * vs))
    return [(mw * a, mh * b, a, b) for a, b in f]


def encode_planes(planes, width, height, sampling, qtabs, tables=(0, 1, 1), factors=None):
    """The component planes of a width x height frame at their own sizes (planes[i].shape = the component's actual size) ->
    the frame's coefficient record, int16"""
    parts = []
    for p, (bw, bh, h, v), t in zip(planes, geometry(width, height, sampling, factors), tables):
        p = np.asarray(p)
        ah, aw = p.shape
        real_w, real_h = -(-aw // 8), -(-ah // 8)
        assert 1 <= real_w <= bw and 1 <= real_h <= bh
        rec = fdct_quant_plane(replicate(p, bw * 8, bh * 8), np.asarray(qtabs).reshape(-1, 64)[t])
        parts.append(apply_dummies(rec, bw, bh, real_w, real_h, h, v).reshape(-1))
    return np.concatenate(parts)


# ---- from RGB
def downsample_h2v1(full):
    """2w x h -> w x h: (a + b + bias) >> 1, bias 0, 1, 0, 1, ... along the output row (jcsample.c h2v1_downsample)"""
    a = np.asarray(full).astype(np.int64)
    bias = np.arange(a.shape[1] // 2) & 1
    return ((a[:, 0::2] + a[:, 1::2] + bias) >> 1).astype(np.uint8)


def downsample_h2v2(full):
    """2w x 2h -> w x h: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ... (jcsample.c h2v2_downsample)"""
    a = np.asarray(full).astype(np.int64)
    bias = 1 + (np.arange(a.shape[1] // 2) & 1)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + bias) >> 2).astype(np.uint8)


def rgb_to_planes(rgb, sampling):
    """uint8 [h, w, 3] -> the component planes libjpeg makes of it, for encode_planes; even width for 422 and 420, even
    height for 420.  The full-size chroma is replicated TO THE RIGHT to whole blocks of the sub-sampled plane BEFORE the
    averaging (jcsample.c expand_right_edge; the bias alternates, so a padded column is not always the copy of the last real
    one): the chroma planes come back ceil(actual width / 8) * 8 wide.  Downward it is the averaged rows that are repeated
    (jcprepct.c), which encode_planes does."""
    from rgb_reference import rgb_to_ycc
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    assert not (sampling in (420, 422) and w % 2) and not (sampling == 420 and h % 2)
    y, cb, cr = rgb_to_ycc(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    if sampling == 400:
        return [y]
    if sampling == 444:
        return [y, cb, cr]
    pw = -(-(w // 2) // 8) * 16
    down = downsample_h2v2 if sampling == 420 else downsample_h2v1
    return [y, down(replicate(cb, pw, h)), down(replicate(cr, pw, h))]
