"""Cases for the libjpeg-exact encoder's tests (tests/test_libjpeg_encode_reference.py on the CPU,
tests/test_gpu_libjpeg_encode.py on the GPU, tests/golden/make_libjpeg_encode_pins.py): a case is named by its parameters,
its samples are made here from a seed or from the golden photograph, and nothing but the pins is stored."""
import hashlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import libjpeg_encode_reference as ler  # noqa: E402

PINS = os.path.join(ROOT, "tests", "golden", "libjpeg_encode_pins.json")

# (width, height, sampling): every rule of the definition is crossed by one of them
PLANE_SIZES = [
    (8, 8, 444), (16, 16, 444), (24, 16, 444), (17, 9, 444), (33, 17, 444), (1, 1, 444), (2, 2, 444),  # whole and ragged blocks
    (8, 8, 400), (17, 9, 400), (3, 2, 400),                                                            # grey
    (16, 16, 420), (2, 2, 420),
    (40, 24, 420),   # dummy luma columns (5 of 6) and a dummy luma row (3 of 4)
    (16, 24, 420),   # a dummy luma row
    (24, 24, 420),   # both, and the corner block that chains through a dummy
    (24, 16, 420),   # a dummy luma column only
    (16, 8, 422), (24, 16, 422),   # 4:2:2: a dummy luma column
    (40, 9, 422),
]
# RGB cases keep to the sizes hvc_rgb_to_yuv accepts (even width under 4:2:2 / 4:2:0, even height under 4:2:0)
RGB_SIZES = [(16, 16, 444), (17, 9, 444), (16, 16, 420), (40, 24, 420), (24, 24, 420), (2, 2, 420), (18, 10, 420), (24, 16, 422),
             (18, 9, 422), (6, 4, 422)]
CONTENTS = ["noise", "gradient", "photo"]
TABLES = ["ones", "q30", "q50", "q75", "q90", "q100", "max"]


def tables(name):
    """[2][64] uint16, zig-zag order: luma, chroma"""
    from video_coding_amd import hvc
    if name == "ones":
        return np.ones((2, 64), dtype=np.uint16)
    if name == "max":
        return np.full((2, 64), 255, dtype=np.uint16)
    q = int(name[1:])
    return np.stack([hvc.quant_table(0, q), hvc.quant_table(1, q)]).astype(np.uint16)


_photo = []


def photo_luma():
    """the luma plane of the golden photograph as the CPU oracle decodes it"""
    if not _photo:
        from oracle import orc
        with open(os.path.join(ROOT, "tests", "golden", "Mouse480.jpg"), "rb") as f:
            d = orc.Decoder(f.read())
        d.decode()
        _photo.append(np.ascontiguousarray(d.get_yuv_frame()[0]))
    return _photo[0]


def content(kind, w, h, seed, n=3):
    """n planes of h x w uint8"""
    if kind == "noise":
        return list(np.random.default_rng(seed).integers(0, 256, size=(n, h, w), dtype=np.uint8))
    if kind == "gradient":
        yy, xx = np.mgrid[0:h, 0:w]
        return [((3 * xx + 5 * yy * (k + 1) + 40 * k) % 256).astype(np.uint8) if k else
                np.clip(2 * xx + 3 * yy + 10, 0, 255).astype(np.uint8) for k in range(n)]
    p = photo_luma()
    return [np.ascontiguousarray(p[40 + 24 * k:40 + 24 * k + h, 100 + 56 * k:100 + 56 * k + w]) for k in range(n)]


def seed_of(w, h, sampling):
    return 9100 + 97 * w + 13 * h + sampling


def component_planes(w, h, sampling, kind):
    """the component planes of a plane case at the sizes the encoder's layout gives them (integer halves)"""
    cw, ch = (w if sampling == 444 else w // 2), (h // 2 if sampling == 420 else h)
    full = content(kind, w, h, seed_of(w, h, sampling))
    if sampling == 400:
        return full[:1]
    return [full[0], np.ascontiguousarray(full[1][:ch, :cw]), np.ascontiguousarray(full[2][:ch, :cw])]


def rgb_image(w, h, sampling, kind):
    return np.ascontiguousarray(np.stack(content(kind, w, h, seed_of(w, h, sampling) + 1), axis=2))


def plane_cases():
    """(name, w, h, sampling, content, tables): every size on noise at q75, every content and table on two sizes"""
    out = [(w, h, s, "noise", "q75") for w, h, s in PLANE_SIZES]
    for w, h, s in [(24, 24, 420), (17, 9, 444)]:
        out += [(w, h, s, k, "q50") for k in CONTENTS]
        out += [(w, h, s, "noise", t) for t in TABLES if t != "q75"]
        out += [(w, h, s, "photo", t) for t in ("ones", "max")]
    return [("planes_%dx%d_%d_%s_%s" % c,) + c for c in dict.fromkeys(out)]


def rgb_cases():
    out = [(w, h, s, "noise", "q75") for w, h, s in RGB_SIZES]
    out += [(40, 24, 420, k, t) for k in ("gradient", "photo") for t in ("ones", "q90")]
    return [("rgb_%dx%d_%d_%s_%s" % c,) + c for c in out]


def reference_record(case):
    """the numpy definition's record of a case"""
    name, w, h, s, kind, tab = case
    if name.startswith("rgb_"):
        planes = ler.rgb_to_planes(rgb_image(w, h, s, kind), s)
    else:
        planes = component_planes(w, h, s, kind)
    return ler.encode_planes(planes, w, h, s, tables(tab))


def have_pillow():
    try:
        import PIL.Image  # noqa: F401
        return True
    except ImportError:
        return False


def pillow_file(case):
    """Pillow's file of a case: our tables through qtables=, no colour step for the plane cases (a YCbCr-mode image whose
    chroma is the component plane with every sample repeated: the averaging of equal samples is the sample)"""
    from PIL import Image
    name, w, h, s, kind, tab = case
    q = tables(tab)
    if name.startswith("rgb_"):
        im = Image.fromarray(rgb_image(w, h, s, kind), "RGB")
    else:
        p = component_planes(w, h, s, kind)
        if s == 400:
            im = Image.fromarray(p[0], "L")
        else:
            fx, fy = (1 if s == 444 else 2), (2 if s == 420 else 1)
            up = [np.repeat(np.repeat(c, fy, axis=0), fx, axis=1)[:h, :w] for c in p[1:]]
            assert all(u.shape == (h, w) for u in up)
            im = Image.fromarray(np.ascontiguousarray(np.stack([p[0]] + up, axis=2)), "YCbCr")
    buf = io.BytesIO()
    kw = {} if s == 400 else {"subsampling": {444: 0, 422: 1, 420: 2}[s]}
    # (Pillow takes a table in natural order and writes it in zig-zag order: file_record checks what the file carries)
    im.save(buf, "JPEG", qtables=[[int(x) for x in t[ler.ZF]] for t in (q[:1] if s == 400 else q)], **kw)
    return buf.getvalue()


def file_record(data, tab=None):
    """the coefficient record of a file through this library's host reader; tab: the tables the file must carry"""
    from video_coding_amd import hvc
    info, coefs = hvc.jpeg_entropy_decode(data)
    if tab is not None:
        q = tables(tab)
        for k in range(info.n_comp):
            assert np.array_equal(np.array(info.qtabs[info.layout[k].qtab][:]), q[min(k, 1)]), "the file does not carry our tables"
    return info, coefs


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
