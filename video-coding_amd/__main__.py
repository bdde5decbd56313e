"""Command line of the path, shaped after the two executables the reference's cram tests drive:

    python -m video_coding_amd model decode frame IN.jpg [OUT.yuv] [-yuv444] [-restart-markers] [-rgb] [-arithmetic model|libjpeg]
                                                                                  jpeg/bin/model.ml:29-45
    python -m video_coding_amd model encode frame IN.yuv WxH OUT.jpg [-quality 75] [-chroma 420] [-restart-interval N] [-arithmetic model|hardcaml|libjpeg]
                                                                                  jpeg/bin/model.ml:86-109
    python -m video_coding_amd model decode frame IN.jpg OUT.ppm -rgb       the RGB image as a binary PPM (P6)
    python -m video_coding_amd model decode frame IN.jpg OUT -scale 2|4|8   at reduced size: the cropped scaled planes (with -rgb: the PPM)
    python -m video_coding_amd model encode frame IN.ppm WxH OUT.jpg -rgb   from a binary PPM of that size
    python -m video_coding_amd model encode frames OUT_DIR IN1.yuv WxH IN2.yuv WxH ... [-quality Q] [-chroma C] [-huffman optimised] [-restart-interval N] [-coder gpu|host] [-arithmetic model|libjpeg]
                                                      raw frames of any sizes in ONE mixed batch call (hvc_jpeg_encode_batch_mixed[_gpu]):
                                                      OUT_DIR/<name>.jpg as `encode frame` writes it; a refused frame is
                                                      printed with its code and the others are still written
    python -m video_coding_amd model encode frames OUT_DIR IN1.ppm WxH IN2.ppm WxH ... -rgb [the other flags as above]
                                                      binary PPMs (P6) of those sizes in ONE call (hvc_jpeg_encode_batch_mixed_rgb[_gpu]):
                                                      OUT_DIR/<name>.jpg as `encode frame -rgb` writes it
    python -m video_coding_amd model decode frames OUT_DIR IN1.jpg IN2.jpg ... [-restart-markers] [-threads 8] [-rgb] [-scale 2|4|8] [-reader gpu|host]
                                                      files of any sizes, samplings and tables in ONE mixed batch call
                                                      (hvc_jpeg_decode_batch_mixed): OUT_DIR/<name>.yuv as `decode frame` writes it;
                                                      -rgb (hvc_jpeg_decode_batch_mixed_rgb): OUT_DIR/<name>.ppm as `decode frame -rgb`
                                                      -scale (hvc_jpeg_decode_batch_mixed_scaled / _scaled_rgb): either as
                                                      `decode frame -scale` writes it
    python -m video_coding_amd model decode frames OUT_DIR IN1.jpg ... -rgb -resize WxH [-filter box|bilinear|bicubic] [-scale N] [-reader gpu|host]
                                                      every image resized to W x H on the GPU, bit-exact to Pillow's
                                                      Image.resize (hvc_jpeg_decode_batch_mixed_resized): OUT_DIR/<name>.ppm
    python -m video_coding_amd model decode frames OUT_DIR IN1.jpg ... -rgb -resize WxH [-box X0,Y0,X1,Y1] [-mirror]
                                                      the window X0,Y0,X1,Y1 of every image (fractions allowed; coordinates of the
                                                      image at 1 / -scale) resized to W x H as Pillow's resize(box=...), -mirror: then
                                                      flipped left to right (hvc_jpeg_decode_batch_mixed_resized_opts)
    python -m video_coding_amd model decode frames OUT_DIR IN1.jpg ... [-rgb] [-resize WxH [-filter ...]] [-reader gpu|host] -arithmetic libjpeg
                                                      the same calls in libjpeg's arithmetic (hvc_set_mixed_arithmetic): every file as
                                                      `decode frame -arithmetic libjpeg` writes it; not with -scale above 1
                                                      (an extension: JFIF colour conversion, hvc_jpeg_decode_rgb / _encode_rgb)
    python -m video_coding_amd oyuv compare {max-difference,mean-difference,mean-square-error,psnr}
                                            {y,u,v,yuv} FILE-1 FILE-2 WxH [-format 420]
                                                                                  tools/src/ocompare.ml:83-135
    python -m video_coding_amd oyuv convert IN.yuv WxH OUT.yuv [W2xH2] [-frames A-B] [-format 420] [-out-format F]
                                            [-src-offset X,Y]    formats 420 422 444 YUY2 UYVY YVYU
                                                                                  tools/src/oconv.ml:58-133
    python -m video_coding_amd simulate decoder IN.jpg [-yuv OUT.yuv] [-blocks N] [-error-tolerance T]
                                                                                  jpeg/bin/simulate.ml:54-80
    python -m video_coding_amd simulate encoder IN.yuv WxH [-chroma 420] [-quality 75] [-blocks N] [-out OUT.jpg]

`simulate decoder` is the reference's decoder simulation (Test_decoder.test) computed by the Hardcaml RTL twin
(hvc_set_arithmetic HVC_ARITH_HARDCAML) instead of a cycle simulation: -yuv writes the RTL's whole frame the way
`model decode frame` writes the model's; for each block in decode order (the first N with -blocks) whose
max_reconstructed_diff from the model is >= T (default 2, test_decoder.ml:27) it prints block_number,
max_reconstructed_diff and the RTL's pixels in the reference's 2-hex-digit pixel_block form, one record per line.
The reference's (comp ...) summary of the model's block is not printed, nor are waveforms (-waves).

`simulate encoder` is the same for the finished half of the RTL encoder datapath (its forward DCT and quantiser,
hvc_set_encode_arithmetic HVC_ARITH_HARDCAML): for each block in encode order (MCU-interleaved, the first N with -blocks)
it prints ((block_number n) (max_coef_diff d)), d the largest difference of a quantised coefficient from the model's;
-out writes the file the RTL arithmetic makes of the frame (its records through this library's entropy coder).
`model encode frame -arithmetic hardcaml` writes that file as well.

    python -m video_coding_amd dct {forward,inverse} [-rom-prec 12] [-transpose-prec 2] [-input-range 200] [-count 1]
    python -m video_coding_amd dct both [-fwd-rom-prec 12] [-fwd-transpose-prec 2] [-inv-rom-prec 12]
                                        [-inv-transpose-prec 2] [-count 1]           jpeg/bin/dct.ml:33-174
    python -m video_coding_amd dct search [-count 10000]
        every subcommand takes -seed S (default 0); forward, inverse and both take -block I

`dct` is the reference's fixed-point DCT tool (hvc_dct_*): blocks come from the library's counter-based generator
(hvc_dct_blocks), not OCaml's Random, so block I of seed S is the same block in every run and every configuration.
-count 1 prints the reference's verbose fields for block 0, -block I for block I; -count N > 1 prints
((max_error E) (worst_block I) (seed S)) over blocks 0 .. N-1.  `search` prints the reference's lines.

Every pixel goes through libhvc_jpeg.so on the GPU (there is no CPU path); output text matches the
reference's (`print_s` of an int / a float), so jpeg/test/*.t expectations can be checked verbatim.
"""
import argparse
import sys

import numpy as np

from . import hvc, yuv


def size_arg(s):
    w, h = s.lower().split("x")
    return int(w), int(h)


def box_arg(s):
    v = tuple(float(x) for x in s.split(","))
    if len(v) != 4:
        raise ValueError("X0,Y0,X1,Y1")
    return v


def read_ppm(path, size):
    """a binary PPM (P6, maxval 255) whose size is `size` -> uint8 [h, w, 3]; ValueError for anything else"""
    raw = open(path, "rb").read()
    fields, pos = [], 0
    while len(fields) < 4:   # magic, width, height, maxval: separated by white space, '#' starts a comment
        while pos < len(raw) and (raw[pos:pos + 1].isspace() or raw[pos:pos + 1] == b"#"):
            if raw[pos:pos + 1] == b"#":
                while pos < len(raw) and raw[pos:pos + 1] != b"\n":
                    pos += 1
            else:
                pos += 1
        end = pos
        while end < len(raw) and not raw[end:end + 1].isspace():
            end += 1
        if end == pos:
            raise ValueError("%s: not a PPM file" % path)
        fields.append(raw[pos:end])
        pos = end
    pos += 1   # the single white-space byte in front of the samples
    try:
        w, h, maxval = (int(f) for f in fields[1:])
    except ValueError:
        raise ValueError("%s: not a PPM file" % path)
    if fields[0] != b"P6" or maxval != 255:
        raise ValueError("%s: not a binary PPM (P6) with maxval 255" % path)
    if (w, h) != tuple(size):
        raise ValueError("%s is %dx%d, not %dx%d" % (path, w, h, size[0], size[1]))
    if len(raw) - pos < 3 * w * h:
        raise ValueError("%s: shorter than its header says" % path)
    return np.frombuffer(raw, dtype=np.uint8, count=3 * w * h, offset=pos).reshape(h, w, 3)


def model_decode_frame(a):
    if a.rgb and a.yuv444:
        raise SystemExit("-rgb and -yuv444 name two different outputs")
    if a.scale != 1 and a.yuv444:
        raise SystemExit("-scale and -yuv444 cannot be combined (the fused 4:4:4 path decodes at full size)")
    if a.arithmetic != "model" and (a.yuv444 or a.scale != 1):
        raise SystemExit("-arithmetic %s decodes at full size into planes or -rgb (no -yuv444, no -scale)" % a.arithmetic)
    data = open(a.bits, "rb").read()
    ctx = hvc.Context(a.device)
    try:
        if a.restart_markers:
            ctx.set_restart_markers(True)
        ctx.set_arithmetic(a.arithmetic)
        if a.rgb:
            info, image = ctx.jpeg_decode_rgb(data) if a.scale == 1 else ctx.jpeg_decode_scaled_rgb(data, a.scale)
            out = np.concatenate([np.frombuffer(b"P6\n%d %d\n255\n" % (info.width, info.height), dtype=np.uint8), image.reshape(-1)])
        elif a.yuv444:
            _, frame = ctx.jpeg_decode_yuv444(data)
            out = frame.reshape(-1)
        elif a.scale != 1:
            info, pixels = ctx.jpeg_decode_scaled(data, a.scale)
            out = hvc.jpeg_get_cropped_planes(info, pixels)  # every component's crop to its scaled actual size
        else:
            info, pixels = ctx.jpeg_decode(data)
            out = hvc.jpeg_get_yuv_frame(info, pixels)  # Decoder.get_yuv_frame: crop to the actual size
    finally:
        ctx.close()
    if a.yuv:
        with open(a.yuv, "wb") as f:
            f.write(out.tobytes())
    else:
        sys.stdout.buffer.write(out.tobytes())


def model_decode_frames_rgb(a, datas):
    """... through one hvc_jpeg_decode_batch_mixed_rgb (-scale: _mixed_scaled_rgb) call: OUT_DIR/<name>.ppm each"""
    import os
    ctx = hvc.Context(a.device)
    try:
        if a.restart_markers:
            ctx.set_restart_markers(True)
        ctx.set_mixed_reader(a.reader)
        ctx.set_mixed_arithmetic(a.arithmetic)
        if a.resize is not None:
            # decoded (at 1 / -scale), converted and resized on the GPU in one hvc_jpeg_decode_batch_mixed_resized call
            # (-box / -mirror: the same window and flip for every file, hvc_jpeg_decode_batch_mixed_resized_opts)
            status, tensor = ctx.jpeg_decode_batch_mixed_resized(datas, size=a.resize, filter=a.filter, scale_denom=a.scale, threads=a.threads,
                                                                 boxes=a.box, mirror=True if a.mirror else None)
            size = type("Size", (), dict(width=a.resize[0], height=a.resize[1]))
            results = [(status[f], size, tensor[f]) for f in range(len(datas))]
        elif a.scale == 1:
            results = ctx.jpeg_decode_batch_mixed_rgb(datas, threads=a.threads)
        else:
            results = ctx.jpeg_decode_batch_mixed_scaled_rgb(datas, a.scale, threads=a.threads)
    finally:
        ctx.close()
    os.makedirs(a.out_dir, exist_ok=True)
    failed = 0
    for path, (status, info, image) in zip(a.bits, results):
        if status != 0:
            failed += 1
            print("%s: %s" % (path, hvc.HvcError(status)), file=sys.stderr)
            continue
        with open(os.path.join(a.out_dir, os.path.splitext(os.path.basename(path))[0] + ".ppm"), "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (info.width, info.height))
            if image is not None:
                fh.write(np.ascontiguousarray(image).tobytes())
    if failed:
        raise SystemExit(1)


def model_decode_frames(a):
    """every file through one hvc_jpeg_decode_batch_mixed call; a file that fails gets a line on stderr and the others are
    still written; the exit status says whether any failed"""
    import os
    if a.arithmetic != "model" and a.scale != 1:   # (before a file is read or a context made, as `decode frame` refuses it)
        raise SystemExit("-arithmetic %s decodes at full size (no -scale): libjpeg's reduced sizes are another definition" % a.arithmetic)
    datas = [open(p, "rb").read() for p in a.bits]
    if a.resize is not None and not a.rgb:
        raise SystemExit("-resize takes RGB images: give -rgb with it")
    if a.resize is not None and (a.resize[0] < 1 or a.resize[1] < 1):
        raise SystemExit("-resize WxH: sizes start at 1")
    if (a.box is not None or a.mirror) and a.resize is None:
        raise SystemExit("-box and -mirror belong to -resize WxH")
    if a.rgb:
        return model_decode_frames_rgb(a, datas)
    lay = hvc.jpeg_mixed_layout(datas) if a.scale == 1 else hvc.jpeg_mixed_scaled_layout(datas, a.scale)
    pixels = np.zeros(max(lay.total_bytes, 8), dtype=np.uint8)
    ctx = hvc.Context(a.device)
    try:
        if a.restart_markers:
            ctx.set_restart_markers(True)
        ctx.set_mixed_reader(a.reader)
        ctx.set_mixed_arithmetic(a.arithmetic)
        if a.scale == 1:
            results = ctx.jpeg_decode_batch_mixed(datas, threads=a.threads, layout=lay, pixels=pixels)
        else:
            results = ctx.jpeg_decode_batch_mixed_scaled(datas, a.scale, threads=a.threads, layout=lay, pixels=pixels)
    finally:
        ctx.close()
    os.makedirs(a.out_dir, exist_ok=True)
    failed = 0
    for f, (path, (status, info, _)) in enumerate(zip(a.bits, results)):
        out = None
        if status == 0:
            off = lay.pixel_offsets[f]
            try:
                rec = pixels[off:off + info.pixel_bytes]
                # (-scale: every component's crop to its scaled actual size, as `decode frame -scale` writes it)
                out = hvc.jpeg_get_yuv_frame(info, rec) if a.scale == 1 else hvc.jpeg_get_cropped_planes(info, rec)
            except hvc.HvcError as e:   # (planes Frame.of_planes has no name for)
                status = e.code
        if out is None:
            failed += 1
            print("%s: %s" % (path, hvc.HvcError(status)), file=sys.stderr)
            continue
        with open(os.path.join(a.out_dir, os.path.splitext(os.path.basename(path))[0] + ".yuv"), "wb") as fh:
            fh.write(out.tobytes())
    if failed:
        raise SystemExit(1)


def model_encode_frame(a):
    w, h = a.size
    if a.rgb:
        try:
            image = read_ppm(a.yuv, a.size)   # (refused here, before any GPU call, when it is not a WxH PPM)
        except ValueError as e:
            raise SystemExit(str(e))
    else:
        y, u, v = yuv.read_frame(a.yuv, w, h, a.chroma)
    ctx = hvc.Context(a.device)
    try:
        if a.arithmetic == "libjpeg":   # a setting of its own (hvc_set_encode_libjpeg)
            ctx.set_encode_libjpeg(True)
        else:
            ctx.set_encode_arithmetic(a.arithmetic)
        ctx.set_huffman_tables(a.huffman)
        ctx.set_restart_interval(a.restart_interval)
        jpg = ctx.jpeg_encode_rgb(image, a.chroma, a.quality) if a.rgb else ctx.jpeg_encode(y, u, v, w, h, a.chroma, a.quality)
    finally:
        ctx.close()
    with open(a.bits, "wb") as f:
        f.write(jpg)


def model_encode_frames(a):
    """every frame through one hvc_jpeg_encode_batch_mixed call (-rgb: hvc_jpeg_encode_batch_mixed_rgb, from PPMs): OUT_DIR/<name>.jpg as `encode frame` writes it; a frame that
    is refused gets a line with its code on stderr and the others are still written; the exit status says whether any was"""
    import os
    if len(a.inputs) % 2:
        raise SystemExit("model encode frames: IN.yuv WxH pairs expected")
    paths = a.inputs[0::2]
    try:
        sizes = [size_arg(s) for s in a.inputs[1::2]]
    except ValueError:
        raise SystemExit("model encode frames: IN.yuv WxH pairs expected")
    specs = [(w, h, a.chroma, a.quality) for w, h in sizes]
    lay = hvc.jpeg_encoder_mixed_rgb_layout(specs) if a.rgb else hvc.jpeg_encoder_mixed_layout(specs)
    frames = []
    for f, (path, (w, h)) in enumerate(zip(paths, sizes)):
        if lay.status[f]:
            frames.append(np.zeros(8, dtype=np.uint8))   # (takes no part)
        elif a.rgb:
            try:
                frames.append(read_ppm(path, (w, h)))    # (refused here, before any GPU call, when it is not a WxH PPM)
            except ValueError as e:
                raise SystemExit(str(e))
        else:
            frames.append(np.concatenate([np.asarray(p, dtype=np.uint8).reshape(-1) for p in yuv.read_frame(path, w, h, a.chroma)]))
    ctx = hvc.Context(a.device)
    try:
        ctx.set_encode_libjpeg(a.arithmetic == "libjpeg")
        ctx.set_huffman_tables(a.huffman)
        ctx.set_restart_interval(a.restart_interval)
        if a.rgb:
            results = ctx.jpeg_encode_batch_mixed_rgb(frames, threads=a.threads, enc_layout=lay, coder=a.coder)
        else:
            results = ctx.jpeg_encode_batch_mixed(frames, threads=a.threads, layout=lay, coder=a.coder)
    finally:
        ctx.close()
    os.makedirs(a.out_dir, exist_ok=True)
    failed = 0
    for path, (status, jpg, _) in zip(paths, results):
        if status:
            failed += 1
            print("%s: %s" % (path, hvc.HvcError(status)), file=sys.stderr)
            continue
        with open(os.path.join(a.out_dir, os.path.splitext(os.path.basename(path))[0] + ".jpg"), "wb") as fh:
            fh.write(jpg)
    if failed:
        raise SystemExit(1)


METRICS = {"max-difference": (yuv.max_difference, str), "mean-difference": (yuv.mean_difference, yuv.float_to_string),
           "mean-square-error": (yuv.mean_square_error, yuv.float_to_string), "psnr": (yuv.psnr, yuv.float_to_string)}


def simulate_decoder(a):
    data = open(a.jpeg, "rb").read()
    info, coefs = hvc.jpeg_entropy_decode(data)
    ctx = hvc.Context(a.device)
    try:
        ctx.set_arithmetic("hardcaml")
        _, pixels = ctx.jpeg_decode(data)
        specs = [dict(blocks_w=L.blocks_w, blocks_h=L.blocks_h, qtab=L.qtab, coef_offset=L.coef_offset)
                 for L in info.layout[:info.n_comp]]
        diff = ctx.decode_divergence(coefs, info.coef_count, info.qtab_array(), specs, 1)[0]
    finally:
        ctx.close()
    if a.yuv:
        with open(a.yuv, "wb") as f:
            f.write(hvc.jpeg_get_yuv_frame(info, pixels).tobytes())
    order = hvc.decode_order_positions(info)
    if a.blocks is not None:
        order = order[:a.blocks]
    ends = np.cumsum([L.blocks_w * L.blocks_h for L in info.layout[:info.n_comp]])
    planes = info.planes(pixels)
    for n, pos in enumerate(order):
        d = int(diff[pos])
        if d < a.error_tolerance:
            continue
        k = int(np.searchsorted(ends, pos, side="right"))
        b = int(pos - (ends[k - 1] if k else 0))
        bw = info.layout[k].blocks_w
        blk = planes[k][(b // bw) * 8:(b // bw) * 8 + 8, (b % bw) * 8:(b % bw) * 8 + 8]
        rows = " ".join("(" + " ".join("%02x" % v for v in row) + ")" for row in blk)
        print("((block_number %d) (max_reconstructed_diff %d) (pixels (%s)))" % (n, d, rows))


def simulate_encoder(a):
    w, h = a.size
    y, u, v = yuv.read_frame(a.yuv, w, h, a.chroma)
    info = hvc.jpeg_encoder_layout(w, h, a.chroma, a.quality)
    rec = hvc.encoder_pixel_record(info, y, u, v, w, h, a.chroma)
    specs = [dict(blocks_w=L.blocks_w, blocks_h=L.blocks_h, qtab=L.qtab, coef_offset=L.coef_offset,
                  plane_offset=L.plane_offset, stride=L.stride) for L in info.layout[:info.n_comp]]
    ctx = hvc.Context(a.device)
    try:
        diff = ctx.encode_divergence(rec, info.pixel_bytes, info.qtab_array(), specs, 1)[0]
        if a.out:
            ctx.set_encode_arithmetic("hardcaml")
            jpg = ctx.jpeg_encode(y, u, v, w, h, a.chroma, a.quality)
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "wb") as f:
            f.write(jpg)
    order = hvc.decode_order_positions(info)
    if a.blocks is not None:
        order = order[:a.blocks]
    for n, pos in enumerate(order):
        print("((block_number %d) (max_coef_diff %d))" % (n, int(diff[pos])))


def oyuv_compare(a):
    w, h = a.size
    f1 = yuv.read_frame(a.file1, w, h, a.format)
    f2 = yuv.read_frame(a.file2, w, h, a.format)
    fn, show = METRICS[a.metric]
    for i in {"y": (0,), "u": (1,), "v": (2,), "yuv": (0, 1, 2)}[a.plane]:
        print(show(fn(f1[i], f2[i])))


def format_arg(s):
    """Yuv_format.arg_type (tools/src/yuv_format.ml:66-77)"""
    try:
        return hvc.YUV_FORMATS[s.upper()]
    except KeyError:
        raise argparse.ArgumentTypeError("Invalid YUV format")


def _two(s):
    """Offset.arg_type / Range.arg_type split on 'x', ',' and '-' (common/src/offset.ml:10-17, range.ml:10-19)"""
    import re
    return re.split("[x,-]", s)


def range_arg(s):
    """Range.arg_type: N = that frame, -B = 0 .. B, A-B (also AxB, A,B)"""
    parts = _two(s)
    try:
        if len(parts) == 1:
            return int(parts[0]), int(parts[0])
        if len(parts) == 2:
            return (0 if parts[0] == "" else int(parts[0])), int(parts[1])
    except ValueError:
        pass
    raise argparse.ArgumentTypeError("Invalid frame size specified")   # (the reference's message, for both types)


def offset_arg(s):
    """Offset.arg_type: XxY, X,Y or X-Y (so no negative offsets on the command line, as in the reference)"""
    parts = _two(s)
    try:
        if len(parts) == 2:
            return int(parts[0]), int(parts[1])
    except ValueError:
        pass
    raise argparse.ArgumentTypeError("Invalid frame size specified")


def oyuv_convert(a):
    """Oconv.main (tools/src/oconv.ml:111-133): skip frames.start frames, then convert frames start .. end; a short read
    ends the run (Plane.End_of_image), whatever has been written stays"""
    size_out = a.out_size or a.size
    fmt_out = a.out_format if a.out_format is not None else a.format
    n_in = hvc.yuv_frame_bytes(a.format, *a.size)
    n_out = hvc.yuv_frame_bytes(fmt_out, *size_out)
    first, last = a.frames
    with (sys.stdin.buffer if a.infile == "-" else open(a.infile, "rb")) as f:
        if first:
            f.read(first * n_in) if a.infile == "-" else f.seek(first * n_in)
        raw = f.read(max(0, last - first + 1) * n_in)   # `for _ = 0 to end_ - start` (oconv.ml:120-131): a reversed range converts nothing
    n = len(raw) // n_in   # (whole frames only: Oconv.input returns false on a short one)
    out = np.zeros(n * n_out, dtype=np.uint8)
    if n:
        ctx = hvc.Context(a.device)
        try:
            ctx.yuv_convert(np.frombuffer(raw, dtype=np.uint8)[:n * n_in], a.format, a.size, out, fmt_out, size_out,
                            offset=a.src_offset, n_frames=n)
        finally:
            ctx.close()
    if a.outfile == "-":
        sys.stdout.buffer.write(out.tobytes())
    else:
        with open(a.outfile, "wb") as f:
            f.write(out.tobytes())


def _sexp_matrix(m, fmt):
    return "(%s)" % " ".join("(%s)" % " ".join(fmt(v) for v in row) for row in np.asarray(m).reshape(8, 8))


def _float(v):
    v = float(v)
    return repr(v) if v != int(v) or abs(v) >= 1e16 else "%d." % int(v)  # OCaml's sexp of a float: round-trips


def _ordered_fmul(a, b):
    """Matrix8x8.fmul (dct.ml:210-218) in float64: each sum from 0.0 in order k = 0..7, products and sums rounded apart"""
    out = np.zeros((8, 8))
    for k in range(8):
        out = out + np.multiply.outer(a[:, k], b[k, :])
    return out


def _dct_print(fields):
    print("(%s)" % "\n ".join("(%s %s)" % kv for kv in fields))


def dct_one(a):
    ctx = hvc.Context(a.device)
    try:
        direction = a.dct_cmd
        if a.block is not None or a.count == 1:
            i = a.block or 0
            x = hvc.dct_blocks(a.seed, a.input_range, i, 1)
            dct = ctx.dct_fixed(direction, a.rom_prec, a.transpose_prec, x)[0]
            ref = ctx.dct_reference(direction, x)[0]
            err = np.abs(dct.astype(np.float64) - ref)
            _dct_print([("inputs", _sexp_matrix(x[0], str)), ("dct", _sexp_matrix(dct, str)),
                        ("ref_dct", _sexp_matrix(ref, _float)), ("max_error", _float(err.max())),
                        ("error", _sexp_matrix(err, _float))])
        else:
            cfg = (direction, a.rom_prec, a.transpose_prec, a.rom_prec, a.transpose_prec)
            e, w = ctx.dct_error_search([cfg], a.seed, a.input_range, 0, a.count)
            print("((max_error %s) (worst_block %d) (seed %d))" % (_float(e[0]), int(w[0]), a.seed))
    finally:
        ctx.close()


def dct_both(a):
    ctx = hvc.Context(a.device)
    try:
        if a.block is not None or a.count == 1:
            i = a.block or 0
            x = hvc.dct_blocks(a.seed, 128, i, 1)
            fwd = ctx.dct_fixed("forward", a.fwd_rom_prec, a.fwd_transpose_prec, x)
            fixed = ctx.dct_fixed("inverse", a.inv_rom_prec, a.inv_transpose_prec, fwd)[0]
            m = hvc.dct_matrix()
            ref = _ordered_fmul(_ordered_fmul(m.T, _ordered_fmul(_ordered_fmul(m, x[0].astype(np.float64)), m.T)), m)
            _dct_print([("inputs", _sexp_matrix(x[0], str)), ("fixed_dct", _sexp_matrix(fixed, str)),
                        ("ref_dct", _sexp_matrix(ref, _float)),
                        ("max_ref_error", _float(np.abs(x[0] - ref).max())),
                        ("max_fixed_error", str(int(np.abs(x[0] - fixed).max())))])
        else:
            cfg = ("round_trip", a.fwd_rom_prec, a.fwd_transpose_prec, a.inv_rom_prec, a.inv_transpose_prec)
            e, w = ctx.dct_error_search([cfg], a.seed, 128, 0, a.count)
            print("((max_error %d) (worst_block %d) (seed %d))" % (int(e[0]), int(w[0]), a.seed))
    finally:
        ctx.close()


def dct_search_configs():
    """the order of jpeg/bin/dct.ml's search: fwd_rom 8..16, fwd_tp 0..5, inv_rom 8..16, inv_tp 0..5"""
    return [(fr, ft, ir, it) for fr in range(8, 17) for ft in range(6) for ir in range(8, 17) for it in range(6)]


def dct_search(a):
    tuples = dct_search_configs()
    ctx = hvc.Context(a.device)
    try:
        e, _ = ctx.dct_error_search([("round_trip",) + t for t in tuples], a.seed, 128, 0, a.count)
    finally:
        ctx.close()
    for t, v in zip(tuples, e):
        print("%2i %2i %2i %2i - %i" % (t + (int(v),)))


def dct_args(top):
    dct = top.add_parser("dct", help="the fixed-point DCT against its float reference, and the precision search")
    sub = dct.add_subparsers(dest="dct_cmd", required=True)
    for name in ("forward", "inverse"):
        p = sub.add_parser(name)
        p.add_argument("-rom-prec", dest="rom_prec", type=int, default=12)
        p.add_argument("-transpose-prec", dest="transpose_prec", type=int, default=2)
        p.add_argument("-input-range", dest="input_range", type=int, default=200)
        p.add_argument("-count", type=int, default=1)
        p.add_argument("-block", type=int, default=None)
        p.set_defaults(fn=dct_one)
    p = sub.add_parser("both")
    for d in ("fwd", "inv"):
        p.add_argument("-%s-rom-prec" % d, dest="%s_rom_prec" % d, type=int, default=12)
        p.add_argument("-%s-transpose-prec" % d, dest="%s_transpose_prec" % d, type=int, default=2)
    p.add_argument("-count", type=int, default=1)
    p.add_argument("-block", type=int, default=None)
    p.set_defaults(fn=dct_both)
    p = sub.add_parser("search")
    p.add_argument("-count", type=int, default=10000)
    p.set_defaults(fn=dct_search)
    for p in sub.choices.values():
        p.add_argument("-seed", type=int, default=0)


def parser():
    ap = argparse.ArgumentParser(prog="python -m video_coding_amd", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-device", type=int, default=0)
    top = ap.add_subparsers(dest="tool", required=True)

    model = top.add_parser("model").add_subparsers(dest="direction", required=True)
    dec = model.add_parser("decode").add_subparsers(dest="what", required=True)
    p = dec.add_parser("frame")
    p.add_argument("bits")
    p.add_argument("yuv", nargs="?")
    p.add_argument("-yuv444", action="store_true", help="4:2:0 file straight to a 4:4:4 frame (fused kernel)")
    p.add_argument("-restart-markers", dest="restart_markers", action="store_true",
                   help="honour DRI + RSTn (hvc_set_restart_markers); off: the model's reading, the first interval only")
    p.add_argument("-rgb", action="store_true", help="write the RGB image as a binary PPM (hvc_jpeg_decode_rgb)")
    p.add_argument("-scale", type=int, default=1, choices=[1, 2, 4, 8],
                   help="decode at 1/2, 1/4 or 1/8 size (hvc_jpeg_decode_scaled / _scaled_rgb): the cropped scaled planes, or with -rgb the PPM")
    p.add_argument("-arithmetic", default="model", choices=["model", "libjpeg"],
                   help="libjpeg: libjpeg's islow inverse DCT and, with -rgb, its fancy upsampling -- the pixels of Pillow, OpenCV "
                        "and djpeg (hvc_set_arithmetic HVC_ARITH_LIBJPEG)")
    p.set_defaults(fn=model_decode_frame)
    p = dec.add_parser("frames", help="files of any sizes, samplings and tables in one mixed batch: OUT_DIR/<name>.yuv each")
    p.add_argument("out_dir")
    p.add_argument("bits", nargs="+")
    p.add_argument("-restart-markers", dest="restart_markers", action="store_true")
    p.add_argument("-threads", type=int, default=8)
    p.add_argument("-rgb", action="store_true", help="write every RGB image as a binary PPM (hvc_jpeg_decode_batch_mixed_rgb)")
    p.add_argument("-reader", choices=["host", "gpu"], default="host",
                   help="who reads the files' Huffman data (hvc_set_mixed_reader): host threads, or the mixed GPU reader; same files either way")
    p.add_argument("-scale", type=int, default=1, choices=[1, 2, 4, 8],
                   help="decode the set at 1/2, 1/4 or 1/8 size (hvc_jpeg_decode_batch_mixed_scaled / _scaled_rgb)")
    p.add_argument("-resize", type=size_arg, default=None, metavar="WxH",
                   help="with -rgb: every image resized to W x H on the GPU, bit-exact to Pillow's Image.resize "
                        "(hvc_jpeg_decode_batch_mixed_resized; -scale: the cheap pre-shrink in front of it)")
    p.add_argument("-filter", choices=["box", "bilinear", "bicubic"], default="bilinear", help="the filter of -resize")
    p.add_argument("-box", type=box_arg, default=None, metavar="X0,Y0,X1,Y1",
                   help="with -resize: the window of every image that is resized, as Pillow's resize(box=...); fractions allowed, "
                        "coordinates of the image at 1 / -scale (hvc_jpeg_decode_batch_mixed_resized_opts)")
    p.add_argument("-mirror", action="store_true", help="with -resize: every resized image flipped left to right")
    p.add_argument("-arithmetic", default="model", choices=["model", "libjpeg"],
                   help="libjpeg: the set in libjpeg's arithmetic, every file as `decode frame -arithmetic libjpeg` writes it "
                        "(hvc_set_mixed_arithmetic HVC_ARITH_LIBJPEG); full size only, no -scale")
    p.set_defaults(fn=model_decode_frames)
    enc = model.add_parser("encode").add_subparsers(dest="what", required=True)
    p = enc.add_parser("frame")
    p.add_argument("yuv")
    p.add_argument("size", type=size_arg)
    p.add_argument("bits")
    p.add_argument("-quality", type=int, default=75)
    p.add_argument("-chroma", type=int, default=420, choices=[420, 422, 444])
    p.add_argument("-arithmetic", default="model", choices=["model", "hardcaml", "libjpeg"],
                   help="hardcaml: the Hardcaml RTL encoder's DCT and quantiser (hvc_set_encode_arithmetic); libjpeg: the "
                        "coefficients libjpeg-turbo writes for these planes (or, with -rgb, this image) and tables (hvc_set_encode_libjpeg)")
    p.add_argument("-huffman", default="default", choices=["default", "optimised"],
                   help="optimised: Huffman tables fitted to the file, Annex K.2 (hvc_set_huffman_tables)")
    p.add_argument("-restart-interval", dest="restart_interval", type=int, default=0,
                   help="N > 0: a DRI segment and an RSTn marker every N MCUs (hvc_set_restart_interval)")
    p.add_argument("-rgb", action="store_true", help="the input is a binary PPM (P6) of that size (hvc_jpeg_encode_rgb)")
    p.set_defaults(fn=model_encode_frame)
    p = enc.add_parser("frames", help="raw frames of any sizes in one mixed batch: OUT_DIR/<name>.jpg each")
    p.add_argument("out_dir")
    p.add_argument("inputs", nargs="+", metavar="IN.yuv WxH")
    p.add_argument("-quality", type=int, default=75)
    p.add_argument("-chroma", type=int, default=420, choices=[420, 422, 444])
    p.add_argument("-huffman", default="default", choices=["default", "optimised"])
    p.add_argument("-arithmetic", default="model", choices=["model", "libjpeg"],
                   help="libjpeg: every file as `encode frame -arithmetic libjpeg` writes it (hvc_set_encode_libjpeg)")
    p.add_argument("-restart-interval", dest="restart_interval", type=int, default=0)
    p.add_argument("-threads", type=int, default=8)
    p.add_argument("-coder", default="host", choices=["gpu", "host"],
                   help="who Huffman-codes the files: host threads, or the mixed GPU coder (hvc_jpeg_encode_batch_mixed_gpu); same bytes")
    p.add_argument("-rgb", action="store_true",
                   help="the inputs are binary PPMs (P6) of those sizes (hvc_jpeg_encode_batch_mixed_rgb[_gpu]): the files of `encode frame -rgb`")
    p.set_defaults(fn=model_encode_frames)

    oyuv =top.add_parser("oyuv").add_subparsers(dest="cmd", required=True)
    p = oyuv.add_parser("compare")
    p.add_argument("metric", choices=sorted(METRICS))
    p.add_argument("plane", choices=["y", "u", "v", "yuv"])
    p.add_argument("file1")
    p.add_argument("file2")
    p.add_argument("size", type=size_arg)
    p.add_argument("-format", type=int, default=420, choices=[420, 422, 444])
    p.set_defaults(fn=oyuv_compare)
    p = oyuv.add_parser("convert")
    p.add_argument("infile")
    p.add_argument("size", type=size_arg)
    p.add_argument("outfile")
    p.add_argument("out_size", type=size_arg, nargs="?")
    p.add_argument("-frames", type=range_arg, default=(0, 0))
    p.add_argument("-format", type=format_arg, default=420)
    p.add_argument("-out-format", dest="out_format", type=format_arg, default=None)
    p.add_argument("-src-offset", dest="src_offset", type=offset_arg, default=(0, 0))
    p.set_defaults(fn=oyuv_convert)

    sim = top.add_parser("simulate").add_subparsers(dest="what", required=True)
    p = sim.add_parser("decoder", help="the Hardcaml RTL decoder's output and its divergence from the model")
    p.add_argument("jpeg")
    p.add_argument("-yuv", default=None)
    p.add_argument("-blocks", type=int, default=None, help="Number of blocks to compare (decode order)")
    p.add_argument("-error-tolerance", dest="error_tolerance", type=int, default=2,
                   help="Allowable error in reconstructed pixels compared to the model reference")
    p.set_defaults(fn=simulate_decoder)
    p = sim.add_parser("encoder", help="the Hardcaml RTL encoder arithmetic's divergence from the model, and its file")
    p.add_argument("yuv")
    p.add_argument("size", type=size_arg)
    p.add_argument("-chroma", type=int, default=420, choices=[420, 422, 444])
    p.add_argument("-quality", type=int, default=75)
    p.add_argument("-blocks", type=int, default=None, help="Number of blocks to compare (encode order)")
    p.add_argument("-out", default=None, help="write the RTL arithmetic's JPEG file")
    p.set_defaults(fn=simulate_encoder)

    dct_args(top)
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    a.fn(a)


if __name__ == "__main__":
    main()
