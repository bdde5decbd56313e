"""ctypes binding of libhvc_jpeg.so (include/hvc_jpeg.h)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("HVC_JPEG_LIB") or os.path.join(_DIR, "libhvc_jpeg.so")  # env override: A/B experiments only
_LIB = None

HVC_MEM_HOST, HVC_MEM_DEVICE = 0, 1

HVC_RESIZE = {"box": 0, "bilinear": 1, "bicubic": 2}  # enum hvc_resize_filter
HVC_RESIZE_MAX_TAPS = 2048
HVC_ELEM = {"float32": 1, "float16": 2, "bfloat16": 3}  # enum hvc_elem: what hvc_normalize_lut makes a table of
ELEM_BYTES = {"float32": 4, "float16": 2, "bfloat16": 2}
HVC_RGB = {"interleaved": 0, "planar": 1}  # enum hvc_rgb_layout: [H, W, 3] / [3, H, W]
HVC_YUV_400 = 400   # luma only, beside 420 / 422 / 444
HVC_HUFF = {"default": 0, "optimised": 1}  # enum hvc_huff_tables
HVC_ARITH = {"model": 0, "hardcaml": 1, "libjpeg": 3}  # enum hvc_arith (2 is not an arithmetic)
HVC_SLOTS = 4       # enum { HVC_SLOTS }
HVC_E_BUSY = -12


class HvcError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = lib().hvc_strerror(code).decode() if _LIB is not None else str(code)
        super().__init__("hvc error %d (%s) %s" % (code, msg, what))


class Component(C.Structure):
    """struct hvc_component"""
    _fields_ = [("blocks_w", C.c_int), ("blocks_h", C.c_int), ("qtab", C.c_int), ("reserved", C.c_int),
                ("coef_offset", C.c_size_t), ("plane_offset", C.c_size_t), ("stride", C.c_size_t)]


class JpegComponent(C.Structure):
    """struct hvc_jpeg_component"""
    _fields_ = [(n, C.c_int) for n in ("identifier", "hscale", "vscale", "decoded_width", "decoded_height",
                                       "actual_width", "actual_height", "dc_table", "ac_table")]


class JpegInfo(C.Structure):
    """struct hvc_jpeg_info"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("n_comp", C.c_int), ("n_qtabs", C.c_int),
                ("comp", JpegComponent * 4), ("layout", Component * 4), ("qtabs", (C.c_uint16 * 64) * 4),
                ("coef_count", C.c_size_t), ("pixel_bytes", C.c_size_t), ("ecs_offset", C.c_size_t)]

    def qtab_array(self):
        return np.array([[self.qtabs[t][i] for i in range(64)] for t in range(self.n_qtabs)], dtype=np.uint16)

    def planes(self, pixels):
        """views of the padded planes inside a frame's pixel record (numpy uint8)"""
        out = []
        for i in range(self.n_comp):
            c, L = self.comp[i], self.layout[i]
            out.append(pixels[L.plane_offset:L.plane_offset + c.decoded_width * c.decoded_height].reshape(
                c.decoded_height, c.decoded_width))
        return out


class HuffSpec(C.Structure):
    """struct hvc_huff_spec: one DHT body (bits[l - 1] codes of length l, then n_vals symbols)"""
    _fields_ = [("bits", C.c_uint8 * 16), ("vals", C.c_uint8 * 256), ("n_vals", C.c_uint16), ("pad", C.c_uint16)]

    def to_pair(self):
        """-> (bits as a list of 16, huffval as a list)"""
        return list(self.bits), list(self.vals[:self.n_vals])

    @classmethod
    def from_pair(cls, bits, vals):
        s = cls()
        bits = list(bits)
        if len(bits) == 17:  # jpeg_opt_writer's bits[0..16] with bits[0] unused
            bits = bits[1:]
        for i, b in enumerate(bits):
            s.bits[i] = b
        for i, v in enumerate(vals):
            s.vals[i] = v
        s.n_vals = len(vals)
        return s


def _spec_pairs(specs, n, status=None):
    """the 4 * n hvc_huff_spec a GPU coder call filled -> per frame its [(bits, vals)] x 4, None for a frame whose status is
    not 0; None where the call had no specs to fill (the default tables)"""
    if specs is None:
        return None
    return [[specs[4 * f + t].to_pair() for t in range(4)] if status is None or status[f] == 0 else None for f in range(n)]


def huff_specs(specs):
    """four (bits, vals) pairs or HuffSpec -> ctypes array of 4 hvc_huff_spec (DC0, DC1, AC0, AC1)"""
    if isinstance(specs, C.Array):
        return specs
    return (HuffSpec * len(specs))(*[s if isinstance(s, HuffSpec) else HuffSpec.from_pair(*s) for s in specs])


class BatchStats(C.Structure):
    """struct hvc_batch_stats"""
    _fields_ = [("wall_ms", C.c_double), ("entropy_ms_sum", C.c_double), ("h2d_ms_sum", C.c_double),
                ("kernel_ms_sum", C.c_double), ("d2h_ms_sum", C.c_double), ("chunks", C.c_int), ("threads", C.c_int),
                ("frames_per_chunk", C.c_int), ("coef_bytes", C.c_uint64), ("host_prep_ms_sum", C.c_double)]


PAGE = os.sysconf("SC_PAGESIZE")


def page_aligned_empty(shape, dtype=np.uint8):
    """a numpy array on whole pages of its own (mmap): what hvc_host_register takes"""
    import mmap
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    buf = mmap.mmap(-1, max((n + PAGE - 1) // PAGE * PAGE, PAGE))
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


class SlotStats(C.Structure):
    """struct hvc_slot_stats"""
    _fields_ = [("h2d_ms", C.c_double), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("h2d_bytes", C.c_uint64),
                ("d2h_bytes", C.c_uint64)]


class ResizeOpts(C.Structure):
    """hvc_resize_opts: a box and a mirror flag per image, a typed output through a table"""
    _fields_ = [("boxes", C.POINTER(C.c_float)), ("mirror", C.POINTER(C.c_uint8)), ("out_elem", C.c_int), ("lut", C.c_void_p)]


class DctConfig(C.Structure):
    _fields_ = [("mode", C.c_int), ("fwd_rom_prec", C.c_int), ("fwd_transpose_prec", C.c_int), ("inv_rom_prec", C.c_int),
                ("inv_transpose_prec", C.c_int)]


class DctError(C.Structure):
    _fields_ = [("max_error", C.c_double), ("worst_block", C.c_uint64)]


# -- the ABI: every function include/hvc_jpeg.h declares, name -> (argtypes[, restype]); restype is int (an hvc_status)
#    where it is not given.  lib() applies the table and SYMBOLS lists it; tests/test_binding_prototypes.py holds it to the header.
_vp, _sz, _i, _u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
_vpp, _szp, _intp, _u64p, _fp = C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_i), C.POINTER(_u64), C.POINTER(C.c_float)
_ip, _hs, _cs, _st = C.POINTER(JpegInfo), C.POINTER(HuffSpec), C.POINTER(Component), C.POINTER(BatchStats)
_FRAMES = [_vp, _vp, _sz, _vp, _i, _cs, _i, _i, _vp, _sz, _i]       # ctx, records in, stride, qtabs, n, comps, n, frames, records out, stride, where
_PLANE_OP = [_vp, _vp, _i, _i, _sz, _vp, _sz, _i, _sz, _sz, _i]    # ctx, src, w, h, stride, dst, stride, planes, plane strides, where
_FILES = [_vpp, _szp, _i]                                          # jpegs, sizes, n_files
_DECODE_BATCH = [_vp] + _FILES + [_i, _i, _vp, _sz, _i, _st]
_ENCODE_BATCH = [_vp, _vpp, _i, _i, _i, _i, _i, _i, _i, _vpp, _szp, _szp, _st]
_ENCODE_BATCH_MIXED = [_vp, _vpp, _ip, _intp, _i, _i, _sz, _vpp, _szp, _szp, _st]
_ENCODE_BATCH_MIXED_RGB = [_vp, _vpp, _szp, _i, _ip, _intp, _i, _i, _sz, _vpp, _szp, _szp, _st]
_COLOUR_MIXED = [_vp, _vp, _szp, _ip, _i, _vp, _szp, _szp, _i, _i]  # ctx, records, offsets, infos, n, rgb, offsets, row strides, layout, where
_RESIZE_MIXED = [_vp, _vp, _szp, _szp, _intp, _intp, _i, _vp, _szp, _szp, _intp, _intp, _i, _i, _i]
_DECODE_BATCH_RESIZED = [_vp] + _FILES + [_i, _sz, _i, _ip, _intp, _intp, _intp, _szp, _szp, _vp, _sz, _i, _i, _i, _st]
_ENCODER_COLUMNS = [_intp, _intp, _intp, _intp, _i]                 # widths, heights, chromas, qualities, n_frames
PROTOTYPES = {
    "hvc_create": ([_vpp, _i],),
    "hvc_destroy": ([_vp], None),
    "hvc_strerror": ([_i], C.c_char_p),
    "hvc_last_hip_error": ([_vp],),
    "hvc_version": ([], C.c_char_p),
    "hvc_host_threads": ([_vp, _intp, _u64p],),
    "hvc_host_threads_probe": ([_i],),
    "hvc_set_host_cpus": ([_vp, C.c_char_p],),
    "hvc_get_host_cpus": ([_vp, C.c_char_p, _sz, _intp],),
    "hvc_set_stream": ([_vp, _vp],),
    "hvc_reset_stream": ([_vp],),
    "hvc_synchronize": ([_vp],),
    "hvc_timer_begin": ([_vp],),
    "hvc_timer_end": ([_vp, _fp],),
    "hvc_set_profiling": ([_vp, _i],),
    "hvc_last_kernel_ms": ([_vp, _fp],),
    "hvc_kernel_ms_history": ([_vp, _fp, _i],),
    "hvc_dequant_idct_recon": ([_vp, _vp, _sz, _vp, _i, _i, _i, _vp, _sz, _sz, _i],),
    "hvc_decode_frames": (_FRAMES,),
    "hvc_decode_frames_yuv444": ([_vp, _vp, _sz, _vp, _i, _cs, _i, _i, _i, _i, _vp, _sz, _i],),
    "hvc_set_decode_kernel": ([_vp, _i],),
    "hvc_set_arithmetic": ([_vp, _i],),
    "hvc_get_arithmetic": ([_vp, _intp],),
    "hvc_decode_frames_divergence": (_FRAMES,),
    "hvc_set_encode_arithmetic": ([_vp, _i],),
    "hvc_get_encode_arithmetic": ([_vp, _intp],),
    "hvc_encode_frames_divergence": (_FRAMES,),
    "hvc_last_wide_blocks": ([_vp, _u64p],),
    "hvc_fdct_quant": ([_vp, _vp, _sz, _sz, _vp, _i, _i, _i, _vp, _sz, _i],),
    "hvc_encode_frames": (_FRAMES,),
    "hvc_encode_frames_recon": (_FRAMES[:-1] + [_vp, _vp, _i],),
    "hvc_upsample420": (_PLANE_OP,),
    "hvc_subsample420": (_PLANE_OP,),
    "hvc_subsample422": (_PLANE_OP,),
    "hvc_upsample422": (_PLANE_OP,),
    "hvc_crop_planes": ([_vp, _vp, _i, _i, _sz, _i, _i, _vp, _i, _i, _sz, _i, _sz, _sz, _i],),
    "hvc_yuv_frame_bytes": ([_i, _i, _i, _szp],),
    "hvc_yuv_convert": ([_vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i],),
    "hvc_jpeg_read_header": ([_vp, _sz, _ip],),
    "hvc_jpeg_entropy_decode": ([_vp, _sz, _ip, _vp],),
    "hvc_jpeg_entropy_decode_restart": ([_vp, _sz, _ip, _vp],),
    "hvc_set_restart_markers": ([_vp, _i],),
    "hvc_jpeg_entropy_decode2": ([_vp, _sz, _ip, _vp, _intp, _vp, _sz, _ip, _vp, _intp],),
    "hvc_jpeg_get_yuv_frame": ([_ip, _vp, _vp, _sz, _szp],),
    "hvc_jpeg_get_cropped_planes": ([_ip, _vp, _vp, _sz, _szp],),
    "hvc_jpeg_decode": ([_vp, _vp, _sz, _ip, _vp, _sz],),
    "hvc_jpeg_decode_yuv444": ([_vp, _vp, _sz, _ip, _vp, _sz],),
    "hvc_jpeg_decode_batch": (_DECODE_BATCH,),
    "hvc_jpeg_decode_batch_yuv444": (_DECODE_BATCH,),
    "hvc_quant_table": ([_i, _i, _vp],),
    "hvc_compare_planes": ([_vp, _vp, _sz, _intp, _u64p, _u64p],),
    "hvc_jpeg_encoder_layout": ([_i, _i, _i, _i, _ip],),
    "hvc_jpeg_decode_batch_gpu": (_DECODE_BATCH[:-1] + [_i, _st],),
    "hvc_jpeg_entropy_decode_gpu": ([_vp] + _FILES + [_vp, _sz, _i, _ip, _intp],),
    "hvc_huffman_encode_frames": ([_vp, _ip, _vp, _sz, _i, _vp, _sz, _vp, _i],),
    "hvc_jpeg_header": ([_ip, _vp, _sz, _szp],),
    "hvc_huffman_code_tables": ([_vp, _i, _i, _vp],),
    "hvc_jpeg_encoder_check": ([_ip],),
    "hvc_jpeg_entropy_encode": ([_ip, _vp, _vp, _sz, _szp],),
    "hvc_jpeg_encode": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _szp],),
    "hvc_set_huffman_tables": ([_vp, _i],),
    "hvc_get_huffman_tables": ([_vp, _intp],),
    "hvc_huffman_spec_from_counts": ([_vp, _hs],),
    "hvc_huffman_optimal_tables": ([_ip, _vp, _hs],),
    "hvc_jpeg_header_tables": ([_ip, _hs, _vp, _sz, _szp],),
    "hvc_jpeg_entropy_encode_tables": ([_ip, _hs, _vp, _vp, _sz, _szp],),
    "hvc_huffman_encode_frames_optimised": ([_vp, _ip, _vp, _sz, _i, _vp, _sz, _vp, _hs, _i],),
    "hvc_set_restart_interval": ([_vp, _i],),
    "hvc_get_restart_interval": ([_vp, _intp],),
    "hvc_jpeg_header_restart": ([_ip, _hs, _i, _vp, _sz, _szp],),
    "hvc_jpeg_entropy_encode_restart": ([_ip, _hs, _i, _vp, _vp, _sz, _szp],),
    "hvc_huffman_optimal_tables_restart": ([_ip, _vp, _i, _hs],),
    "hvc_huffman_encode_frames_restart": ([_vp, _ip, _vp, _sz, _i, _i, _i, _vp, _sz, _vp, _hs, _i],),
    "hvc_jpeg_encode_batch": (_ENCODE_BATCH,),
    "hvc_jpeg_encode_batch_gpu": (_ENCODE_BATCH,),
    "hvc_yuv_to_rgb": ([_vp, _vp, _sz, _cs, _i, _i, _i, _i, _i, _i, _vp, _sz, _sz, _i, _i],),
    "hvc_rgb_to_yuv": ([_vp, _vp, _sz, _sz, _i, _i, _i, _i, _i, _vp, _sz, _cs, _i],),
    "hvc_decode_frames_rgb": ([_vp, _vp, _sz, _vp, _i, _cs, _i, _i, _i, _i, _i, _vp, _sz, _sz, _i, _i],),
    "hvc_jpeg_decode_rgb": ([_vp, _vp, _sz, _ip, _vp, _sz, _sz, _i],),
    "hvc_jpeg_decode_batch_rgb": ([_vp] + _FILES + [_i, _i, _i, _vp, _sz, _sz, _i, _i, _st],),
    "hvc_jpeg_encode_rgb": ([_vp, _vp, _sz, _i, _i, _i, _i, _i, _vp, _sz, _szp],),
    "hvc_set_mixed_arithmetic": ([_vp, _i],),
    "hvc_get_mixed_arithmetic": ([_vp, _intp],),
    "hvc_set_encode_libjpeg": ([_vp, _i],),
    "hvc_get_encode_libjpeg": ([_vp, _intp],),
    "hvc_jpeg_scaled_info": ([_ip, _i, _ip],),
    "hvc_decode_frames_scaled": ([_vp, _vp, _sz, _vp, _i, _cs, _i, _i, _i, _vp, _sz, _i],),
    "hvc_jpeg_decode_scaled": ([_vp, _vp, _sz, _i, _ip, _vp, _sz],),
    "hvc_jpeg_decode_scaled_rgb": ([_vp, _vp, _sz, _i, _ip, _vp, _sz, _sz, _i],),
    "hvc_jpeg_decode_batch_scaled": ([_vp] + _FILES + [_i, _i, _i, _i, _vp, _sz, _i, _st],),
    "hvc_jpeg_mixed_layout": (_FILES + [_sz, _ip, _intp, _szp, _szp],),
    "hvc_decode_frames_mixed": ([_vp, _vp, _szp, _ip, _i, _vp, _szp, _i],),
    "hvc_jpeg_decode_batch_mixed": ([_vp] + _FILES + [_i, _sz, _ip, _intp, _szp, _vp, _sz, _i, _st],),
    "hvc_set_mixed_reader": ([_vp, _i],),
    "hvc_get_mixed_reader": ([_vp, _intp],),
    "hvc_last_mixed_reader_files": ([_vp, _u64p, _u64p],),
    "hvc_jpeg_entropy_decode_gpu_mixed": ([_vp] + _FILES + [_vp, _intp, _vp, _szp, _sz, _i, _intp],),
    "hvc_jpeg_mixed_rgb_layout": (_FILES + [_i, _sz, _sz, _ip, _intp, _szp, _szp, _szp],),
    "hvc_yuv_to_rgb_mixed": (_COLOUR_MIXED,),
    "hvc_decode_frames_mixed_rgb": (_COLOUR_MIXED,),
    "hvc_jpeg_decode_batch_mixed_rgb": ([_vp] + _FILES + [_i, _sz, _ip, _intp, _szp, _szp, _vp, _sz, _i, _i, _st],),
    "hvc_jpeg_mixed_scaled_layout": (_FILES + [_i, _sz, _ip, _ip, _intp, _szp, _szp],),
    "hvc_decode_frames_mixed_scaled": ([_vp, _vp, _szp, _ip, _i, _i, _vp, _szp, _i],),
    "hvc_jpeg_decode_batch_mixed_scaled": ([_vp] + _FILES + [_i, _sz, _i, _ip, _intp, _szp, _vp, _sz, _i, _st],),
    "hvc_jpeg_mixed_scaled_rgb_layout": (_FILES + [_i, _i, _sz, _sz, _ip, _ip, _intp, _szp, _szp, _szp],),
    "hvc_jpeg_decode_batch_mixed_scaled_rgb": ([_vp] + _FILES + [_i, _sz, _i, _ip, _intp, _szp, _szp, _vp, _sz, _i, _i, _st],),
    "hvc_jpeg_encoder_mixed_layout": (_ENCODER_COLUMNS + [_sz, _ip, _intp, _szp, _szp, _szp, _szp],),
    "hvc_encode_frames_mixed": ([_vp, _vp, _szp, _ip, _i, _vp, _szp, _i],),
    "hvc_jpeg_encode_batch_mixed": (_ENCODE_BATCH_MIXED,),
    "hvc_huffman_encode_frames_mixed": ([_vp, _ip, _vp, _szp, _i, _i, _vp, _sz, _vp, _intp, _hs, _i],),
    "hvc_jpeg_encode_batch_mixed_gpu": (_ENCODE_BATCH_MIXED,),
    "hvc_last_mixed_coder_files": ([_vp, _u64p, _u64p],),
    "hvc_jpeg_encoder_mixed_rgb_layout": (_ENCODER_COLUMNS + [_i, _sz, _sz, _ip, _intp, _szp, _szp, _szp, _szp, _szp, _szp, _szp],),
    "hvc_rgb_to_yuv_mixed": (_COLOUR_MIXED,),
    "hvc_encode_frames_mixed_rgb": ([_vp, _vp, _szp, _szp, _i, _ip, _i, _vp, _szp, _i],),
    "hvc_jpeg_encode_batch_mixed_rgb": (_ENCODE_BATCH_MIXED_RGB,),
    "hvc_jpeg_encode_batch_mixed_rgb_gpu": (_ENCODE_BATCH_MIXED_RGB,),
    "hvc_rgb_resize_mixed": (_RESIZE_MIXED,),
    "hvc_jpeg_decode_batch_mixed_resized": (_DECODE_BATCH_RESIZED,),
    "hvc_rgb_resize_mixed_opts": (_RESIZE_MIXED + [C.POINTER(ResizeOpts)],),
    "hvc_jpeg_decode_batch_mixed_resized_opts": (_DECODE_BATCH_RESIZED + [C.POINTER(ResizeOpts)],),
    "hvc_normalize_lut": ([_fp, _fp, _i, _vp],),
    "hvc_checksum_records": ([_vp, _vp, _sz, _sz, _i, _vp, _i],),
    "hvc_host_alloc": ([_vp, _sz, _vpp],),
    "hvc_host_free": ([_vp, _vp],),
    "hvc_host_register": ([_vp, _vp, _sz],),
    "hvc_host_unregister": ([_vp, _vp],),
    "hvc_decode_frames_submit": ([_vp, _i] + _FRAMES[1:],),
    "hvc_encode_frames_submit": ([_vp, _i] + _FRAMES[1:],),
    "hvc_wait": ([_vp, _i],),
    "hvc_slot_query": ([_vp, _i, _intp],),
    "hvc_slot_last_stats": ([_vp, _i, C.POINTER(SlotStats)],),
    "hvc_dct_rom": ([_i, _vp],),
    "hvc_dct_matrix": ([_vp],),
    "hvc_dct_blocks": ([_u64, _i, _u64, _sz, _vp],),
    "hvc_dct_fixed": ([_vp, _i, _i, _i, _vp, _vp, _sz, _i],),
    "hvc_dct_reference": ([_vp, _i, _vp, _vp, _sz, _i],),
    "hvc_dct_error_search": ([_vp, C.POINTER(DctConfig), _sz, _u64, _i, _u64, _u64, C.POINTER(DctError)],),
    "hvc_device_alloc": ([_vp, _sz, _vpp],),
    "hvc_device_free": ([_vp, _vp],),
    "hvc_memcpy_h2d": ([_vp, _vp, _vp, _sz],),
    "hvc_memcpy_d2h": ([_vp, _vp, _vp, _sz],),
}
SYMBOLS = list(PROTOTYPES)


def build(force=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_DIR, "csrc", f) for f in os.listdir(os.path.join(_DIR, "csrc"))]
    srcs.append(os.path.join(os.path.dirname(_DIR), "include", "hvc_jpeg.h"))
    stale = not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-s", "-C", os.path.join(_DIR, "csrc")] + (["-B"] if force else []))
    return _SO


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise ImportError("libhvc_jpeg.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C video-coding_amd/csrc` (there is no CPU fallback)")
        if "torch" not in sys.modules:
            # A process that also uses PyTorch-ROCm must run ONE HIP runtime: torch bundles
            # its own libamdhip64 (same SONAME as /opt/rocm's).  Loading torch first makes the
            # dynamic linker resolve this library's dependency to the copy torch already
            # mapped; the other order leaves torch without a usable device.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(_SO)
        for name, proto in PROTOTYPES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise ImportError("%s lacks %s, which include/hvc_jpeg.h declares: rebuild it from this tree" % (_SO, name))
            fn.argtypes = proto[0]
            if len(proto) > 1:
                fn.restype = proto[1]
        _LIB = L
    return _LIB


KERNEL_SRCS = ("hvc_kernels.hip", "hvc_kernels.h", "hvc_idct_spec.h")   # csrc/Makefile KERNEL_SRCS, in that order


def kernel_build_id():
    """the kernel id the loaded library reports (hvc_version: "... kernels <id>")"""
    return lib().hvc_version().decode().rsplit(" ", 1)[-1]


def kernel_source_id():
    """the same id computed from the sources in the tree (None where they are not there)"""
    import hashlib
    h = hashlib.sha256()
    try:
        for f in KERNEL_SRCS:
            with open(os.path.join(_DIR, "csrc", f), "rb") as fh:
                h.update(fh.read())
    except OSError:
        return None
    return h.hexdigest()[:12]


def _enum(table, v):
    """a name of `table`, or the number itself"""
    return table[v] if isinstance(v, str) else int(v)


def _rgb_layout(layout):
    return _enum(HVC_RGB, layout)


def _resize_filter(filter):
    return _enum(HVC_RESIZE, filter)


ARITH_NAMES = {v: k for k, v in HVC_ARITH.items()}   # what the getters answer: the name, or the number where it has none
HUFF_NAMES = {v: k for k, v in HVC_HUFF.items()}


def elem_name(dtype):
    """"float32" / "float16" / "bfloat16" of a name, a numpy dtype or a torch dtype"""
    name = str(dtype).replace("torch.", "").replace("<class 'numpy.", "").replace("'>", "")
    name = {"half": "float16", "float": "float32"}.get(name, name)
    if name not in HVC_ELEM:
        raise ValueError("dtype %r: one of float32, float16, bfloat16" % (dtype,))
    return name


def normalize_lut(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), dtype="float32"):
    """hvc_normalize_lut: the [3, 256] table ((float)v / 255.0f - mean[c]) / std[c] in IEEE single, rounded once to dtype --
    torchvision's ToTensor() + Normalize(mean, std) on the CPU, bit for bit.  numpy float32 / float16; bfloat16: the raw bits as
    uint16 (numpy has no such type; torch.from_numpy(lut).view(torch.bfloat16) reads them)."""
    name = elem_name(dtype)
    out = np.zeros((3, 256), dtype={"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}[name])
    m, s = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
    _chk(lib().hvc_normalize_lut(m, s, HVC_ELEM[name], out.ctypes.data), "hvc_normalize_lut")
    return out


def resize_opts(n, boxes=None, mirror=None, dtype=None, mean=None, std=None, lut=None):
    """(ResizeOpts or None, what must stay alive during the call, bytes per output element, dtype name or None) of the keyword
    arguments the resizing calls share.  boxes: n x (x0, y0, x1, y1), or one box for every image; mirror: n flags, or one;
    dtype with mean / std (defaults 0 and 1): a table made by normalize_lut; lut: a [3, 256] array of 2- or 4-byte elements of
    the caller's own (dtype then only names what the result is viewed as).  Nothing given: (None, [], 1, None)."""
    if boxes is None and mirror is None and dtype is None and lut is None:
        assert mean is None and std is None, "mean= / std= come with dtype="
        return None, [], 1, None
    o, keep, name = ResizeOpts(), [], None
    if boxes is not None:
        b = np.asarray(boxes, dtype=np.float32)
        b = np.tile(b.reshape(1, 4), (max(n, 1), 1)) if b.ndim == 1 else np.ascontiguousarray(b.reshape(n, 4))
        keep.append(b)
        o.boxes = b.ctypes.data_as(C.POINTER(C.c_float))
    if mirror is not None:
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(mirror).astype(bool).astype(np.uint8).reshape(-1), (max(n, 1),)))
        keep.append(m)
        o.mirror = m.ctypes.data_as(C.POINTER(C.c_uint8))
    if lut is not None:
        assert mean is None and std is None, "lut= is the table itself: no mean= / std="
        t = np.ascontiguousarray(lut)
        assert t.shape == (3, 256) and t.dtype.itemsize in (2, 4), "lut: [3, 256] of 2- or 4-byte elements"
        name = elem_name(dtype) if dtype is not None else None
        assert name is None or ELEM_BYTES[name] == t.dtype.itemsize
    elif dtype is not None:
        name = elem_name(dtype)
        t = normalize_lut(mean if mean is not None else (0.0,) * 3, std if std is not None else (1.0,) * 3, name)
    else:
        assert mean is None and std is None, "mean= / std= come with dtype="
        return o, keep, 1, None
    keep.append(t)
    o.out_elem, o.lut = t.dtype.itemsize, t.ctypes.data
    return o, keep, t.dtype.itemsize, name


def typed_view(buf, name, itemsize):
    """a byte buffer (numpy / torch) seen as elements of dtype `name` (None: unsigned integers of itemsize bytes; bfloat16 in
    numpy: uint16)"""
    if hasattr(buf, "data_ptr"):
        import torch
        return buf.view({None: {1: torch.uint8, 2: torch.int16, 4: torch.int32}[itemsize], "float32": torch.float32,
                         "float16": torch.float16, "bfloat16": torch.bfloat16}[name])
    return buf.view({None: {1: np.uint8, 2: np.uint16, 4: np.uint32}[itemsize], "float32": np.float32, "float16": np.float16,
                     "bfloat16": np.uint16}[name])


def rgb_shape(layout, width, height):
    """the shape of one tight image: (h, w, 3) interleaved, (3, h, w) planar"""
    return (3, height, width) if _rgb_layout(layout) == 1 else (height, width, 3)


def rgb_chroma_window(sampling, width, height):
    """the chroma samples the RGB image of a width x height frame reads: ceil halves (include/hvc_jpeg.h, RGB)"""
    return (width if sampling == 444 else (width + 1) // 2, (height + 1) // 2 if sampling == 420 else height)


def _chk(code, what=""):
    if code != 0:
        raise HvcError(code, what)


def _addr(x):
    """host numpy array or device torch tensor / raw int address -> (address, where)"""
    if isinstance(x, np.ndarray):
        return x.ctypes.data, HVC_MEM_HOST
    if isinstance(x, int):
        return x, HVC_MEM_DEVICE
    if hasattr(x, "data_ptr"):
        return x.data_ptr(), (HVC_MEM_DEVICE if x.is_cuda else HVC_MEM_HOST)
    raise TypeError(type(x))


def _same_space(a, a_name, b, b_name):
    """(address of a, address of b, where) of two buffers a call takes in ONE memory space"""
    aa, w1 = _addr(a)
    ba, w2 = _addr(b)
    assert w1 == w2, "%s and %s must live in the same memory space" % (a_name, b_name)
    return aa, ba, w1


def _infos_array(infos):
    """a list of JpegInfo as the ctypes array a call takes (never of length 0: the array of an empty set is one unused entry)"""
    return infos if isinstance(infos, C.Array) else (JpegInfo * max(len(infos), 1))(*infos)


def _zeroed_bytes(n, device):
    """the zero-filled buffer a batch call decodes into when the caller brings none: n bytes (8 at least), a torch cuda tensor
    with `device`, a numpy array without"""
    if device:
        import torch
        return torch.zeros(max(n, 8), dtype=torch.uint8, device="cuda")
    return np.zeros(max(n, 8), dtype=np.uint8)


def _flat_bytes(frames):
    """raw frames (bytes / bytearray / uint8 arrays of any shape) as flat uint8 arrays, without a copy where none is needed"""
    return [np.frombuffer(f, dtype=np.uint8) if isinstance(f, (bytes, bytearray)) else
            np.ascontiguousarray(f, dtype=np.uint8).reshape(-1) for f in frames]


def _capacity(buf):
    """the elements of a numpy array or a torch tensor"""
    return buf.numel() if hasattr(buf, "numel") else buf.size


HVC_DCT = {"forward": 0, "inverse": 1, "round_trip": 2}   # HVC_DCT_FORWARD / _INVERSE / _ROUND_TRIP
DCT_ROM_PREC_MAX, DCT_TP_MAX = 16, 8                      # hvc_dct_spec.h
DCT_FWD_IN_MAX, DCT_INV_IN_MAX = 2048, 32768


def _dct_direction(d):
    return _enum(HVC_DCT, d)


def dct_rom(rom_prec):
    """the forward ROM of rom_prec, round_nearest(M * 2^rom_prec) (hvc_dct_rom) -> int32 [8, 8]"""
    out = np.zeros((8, 8), dtype=np.int32)
    _chk(lib().hvc_dct_rom(int(rom_prec), out.ctypes.data), "hvc_dct_rom")
    return out


def dct_matrix():
    """the float64 forward matrix M, the static x86 one of dct.ml (hvc_dct_matrix) -> float64 [8, 8]"""
    out = np.zeros((8, 8), dtype=np.float64)
    _chk(lib().hvc_dct_matrix(out.ctypes.data), "hvc_dct_matrix")
    return out


def dct_blocks(seed, range_, first, n):
    """the search's generated blocks first .. first + n - 1 (hvc_dct_blocks) -> int32 [n, 8, 8]"""
    out = np.zeros((n, 8, 8), dtype=np.int32)
    _chk(lib().hvc_dct_blocks(int(seed), int(range_), int(first), int(n), out.ctypes.data), "hvc_dct_blocks")
    return out


def dct_configs(cfgs):
    """[(mode, fwd_rom, fwd_tp, inv_rom, inv_tp), ...] (mode a name of HVC_DCT or its number) -> DctConfig array"""
    arr = (DctConfig * len(cfgs))()
    for a, c in zip(arr, cfgs):
        a.mode = _dct_direction(c[0])
        a.fwd_rom_prec, a.fwd_transpose_prec, a.inv_rom_prec, a.inv_transpose_prec = (int(v) for v in c[1:5])
    return arr


def components(specs):
    """specs: list of dicts(blocks_w, blocks_h, qtab, coef_offset, plane_offset, stride)"""
    arr = (Component * len(specs))()
    for a, s in zip(arr, specs):
        a.blocks_w, a.blocks_h, a.qtab = s["blocks_w"], s["blocks_h"], s.get("qtab", 0)
        a.coef_offset, a.plane_offset = s.get("coef_offset", 0), s.get("plane_offset", 0)
        a.stride = s.get("stride", s["blocks_w"] * 8)
    return arr


def layout_alignment(planes_bw_bh_qtab):
    """Where a resident batch's planes and frames should start (bytes).  Measured on MI355X (profiles/r05l_alignment_sweep.txt,
    r05m / r05n_layout_ab.txt, profiles/ANALYSIS.md section 7): with every plane of every frame -- pixels and coefficients -- on a
    64 KiB boundary k_decode_packed gains 0.4 ... 1.0 points of the HBM peak on 1080p 4:2:0 frames, whose second chroma plane
    otherwise starts 2 KiB off a 4 KiB boundary; 2 MiB boundaries give k_encode 0.6 ... 1.2 points on 4K 4:2:0 frames -- and cost 1080p
    frames 1.3 points, because they nearly double that batch's footprint.  So: the larger of 2 MiB / 64 KiB whose padding stays
    under 3 % of the frame.  The padding is neither read nor written."""
    tight = sum(bw * bh * 64 for bw, bh, _ in planes_bw_bh_qtab)
    for a in (2 << 20, 65536):
        if sum((bw * bh * 64 + a - 1) // a * a for bw, bh, _ in planes_bw_bh_qtab) <= 1.03 * tight:
            return a
    return 65536


def frame_layout(planes_bw_bh_qtab, align=1):
    """Frame record: component planes back to back, each starting on an `align`-byte boundary (1 = tight, the default;
    "auto" = layout_alignment()), pixel planes and coefficient planes alike; the frame strides are rounded up the same way.
    Returns (specs, coef elements per frame, pixel bytes per frame)."""
    if align == "auto":
        align = layout_alignment(planes_bw_bh_qtab)
    up = lambda x: (x + align - 1) // align * align
    specs, co, po = [], 0, 0
    for bw, bh, qt in planes_bw_bh_qtab:
        co, po = up(co * 2) // 2, up(po)
        specs.append(dict(blocks_w=bw, blocks_h=bh, qtab=qt, coef_offset=co, plane_offset=po, stride=bw * 8))
        co += bw * bh * 64
        po += bw * bh * 64
    return specs, up(co * 2) // 2, up(po)


def tight_records(t, specs, which):
    """the planes of a batch laid out by frame_layout(..., align) gathered into tight records (torch tensor [n, stride] ->
    [n, sum of the planes]): which = "plane_offset" (pixel bytes) or "coef_offset" (int16 elements) -- what the K5 golden
    checksums are defined on, whatever the resident layout"""
    import torch
    return torch.cat([t[:, s[which]:s[which] + s["blocks_w"] * s["blocks_h"] * 64] for s in specs], dim=1).contiguous()


def spread_records(tight, specs_tight, specs, stride, which):
    """the inverse: tight records [n, ...] into a zeroed batch [n, stride] laid out by `specs`"""
    import torch
    out = torch.zeros((tight.shape[0], stride), dtype=tight.dtype, device=tight.device)
    for a, b in zip(specs_tight, specs):
        n = a["blocks_w"] * a["blocks_h"] * 64
        out[:, b[which]:b[which] + n] = tight[:, a[which]:a[which] + n]
    return out


def decode_order_positions(info):
    """For every block in the model's decode order (decode_seq, jpeg/model/src/decoder.ml:374-397: macroblocks in raster
    order, inside one the components in turn, inside a component its vscale x hscale blocks row by row) its index in the
    per-frame divergence array of hvc_decode_frames_divergence (the components' blocks back to back, each plane row-major)
    -> int64 array.  Block n of this order is the reference's block_number n (hardcaml/test/test_decoder.ml)."""
    n = info.n_comp
    bw = [info.comp[k].decoded_width // 8 for k in range(n)]
    bh = [info.comp[k].decoded_height // 8 for k in range(n)]
    blk0 = np.concatenate([[0], np.cumsum([w * h for w, h in zip(bw, bh)])])
    h0, v0 = info.comp[0].hscale, info.comp[0].vscale
    if n == 0 or not h0 or not v0:
        return np.zeros(0, dtype=np.int64)
    mbw, mbh = info.comp[0].decoded_width // (8 * h0), info.comp[0].decoded_height // (8 * v0)
    parts = []
    for k in range(n):
        hs, vs = info.comp[k].hscale, info.comp[k].vscale
        # [mbh, mbw, vs, hs] positions of this component's blocks inside each macroblock
        my, mx, y, x = np.meshgrid(np.arange(mbh), np.arange(mbw), np.arange(vs), np.arange(hs), indexing="ij")
        parts.append((blk0[k] + (my * vs + y) * bw[k] + mx * hs + x).reshape(mbh, mbw, vs * hs))
    return np.concatenate(parts, axis=2).reshape(-1).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)


# -- host front end / back end (no GPU needed) ------------------------------------------------
def jpeg_read_header(data: bytes):
    """Decoder.Header.decode + Decoder.init geometry -> JpegInfo"""
    info = JpegInfo()
    _chk(lib().hvc_jpeg_read_header(data, len(data), C.byref(info)), "hvc_jpeg_read_header")
    return info


class _FileSetLayout:
    """what the four hvc_jpeg_mixed*_layout calls make of a list of files, the part they share: jpegs (the files), ptrs and
    sizes (ctypes arrays: what the batch calls take), infos (ctypes array of JpegInfo), status (ctypes array, one hvc_status
    per file) and total_bytes; len() = the number of files.  Each class names its call, the arguments between n_files and
    infos, and the size_t arrays the call fills behind status."""

    def _lay_out(self, name, jpegs, middle, arrays, scaled=False):
        """name(ptrs, sizes, n, *middle, infos, [scaled,] status, *arrays, &total_bytes)"""
        n = len(jpegs)
        self.jpegs = list(jpegs)
        self.ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(j), C.c_void_p) for j in self.jpegs])
        self.sizes = (C.c_size_t * n)(*[len(j) for j in self.jpegs])
        self.infos = (JpegInfo * n)()
        out_infos = [self.infos]
        if scaled:
            self.scaled = (JpegInfo * n)()
            out_infos.append(self.scaled)
        self.status = (C.c_int * n)()
        for a in arrays:
            setattr(self, a, (C.c_size_t * n)())
        total = C.c_size_t(0)
        _chk(getattr(lib(), name)(self.ptrs, self.sizes, n, *middle, *out_infos, self.status, *[getattr(self, a) for a in arrays],
                                  C.byref(total)), name)
        self.total_bytes = total.value

    def __len__(self):
        return len(self.jpegs)


class MixedLayout(_FileSetLayout):
    """what hvc_jpeg_mixed_layout makes of a list of files: infos (ctypes array of JpegInfo), status and pixel_offsets (ctypes
    arrays, one entry per file) and total_bytes -- the size of the buffer that holds every good file's pixel record"""

    def __init__(self, jpegs, align=0):
        self._lay_out("hvc_jpeg_mixed_layout", jpegs, (align,), ("pixel_offsets",))


def mixed_coef_offsets(layout):
    """where jpeg_entropy_decode_gpu_mixed puts the coefficient record of every file of a MixedLayout: (offsets, a ctypes array
    of int16 elements, each on a whole block; the elements of all records)"""
    n = len(layout)
    offs, total = (C.c_size_t * n)(), 0
    for f in range(n):
        offs[f] = total
        if layout.status[f] == 0:
            total += (layout.infos[f].coef_count + 63) // 64 * 64
    return offs, total


def jpeg_mixed_layout(jpegs, align=0):
    """headers of a list of files (bytes) -> MixedLayout; align: a power of two >= 8, 0 = 256"""
    return MixedLayout(jpegs, align)


class MixedRgbLayout(_FileSetLayout):
    """what hvc_jpeg_mixed_rgb_layout makes of a list of files: infos, status (nonzero also for a sampling without an RGB
    image), rgb_offsets and rgb_row_strides (ctypes arrays, one entry per file) and total_bytes -- the size of the buffer
    that holds every good file's RGB image"""

    def __init__(self, jpegs, layout="interleaved", align=0, row_align=0):
        self.layout = _rgb_layout(layout)
        self._lay_out("hvc_jpeg_mixed_rgb_layout", jpegs, (self.layout, align, row_align), ("rgb_offsets", "rgb_row_strides"))


def jpeg_mixed_rgb_layout(jpegs, layout="interleaved", align=0, row_align=0):
    """headers of a list of files (bytes) -> MixedRgbLayout; align / row_align: powers of two, 0 = 256 / 1 (tight rows)"""
    return MixedRgbLayout(jpegs, layout, align, row_align)


class MixedScaledLayout(_FileSetLayout):
    """what hvc_jpeg_mixed_scaled_layout makes of a list of files: infos (FULL-size: the batch call's input), scaled (the infos
    of the output records), status, pixel_offsets and total_bytes -- the size of the buffer that holds every good file's
    scaled pixel record"""

    def __init__(self, jpegs, scale_denom, align=0):
        self.scale_denom = int(scale_denom)
        self._lay_out("hvc_jpeg_mixed_scaled_layout", jpegs, (self.scale_denom, align), ("pixel_offsets",), scaled=True)


def jpeg_mixed_scaled_layout(jpegs, scale_denom, align=0):
    """headers of a list of files (bytes) -> MixedScaledLayout; scale_denom 1, 2, 4, 8; align: a power of two >= 8, 0 = 256"""
    return MixedScaledLayout(jpegs, scale_denom, align)


class MixedScaledRgbLayout(_FileSetLayout):
    """what hvc_jpeg_mixed_scaled_rgb_layout makes of a list of files: infos (FULL-size), scaled (image f is scaled[f].width x
    .height), status, rgb_offsets, rgb_row_strides and total_bytes"""

    def __init__(self, jpegs, scale_denom, layout="interleaved", align=0, row_align=0):
        self.scale_denom = int(scale_denom)
        self.layout = _rgb_layout(layout)
        self._lay_out("hvc_jpeg_mixed_scaled_rgb_layout", jpegs, (self.scale_denom, self.layout, align, row_align),
                      ("rgb_offsets", "rgb_row_strides"), scaled=True)


def jpeg_mixed_scaled_rgb_layout(jpegs, scale_denom, layout="interleaved", align=0, row_align=0):
    """headers of a list of files (bytes) -> MixedScaledRgbLayout; align / row_align: powers of two, 0 = 256 / 1 (tight rows)"""
    return MixedScaledRgbLayout(jpegs, scale_denom, layout, align, row_align)


def rgb_view(buf, offset, row_stride, width, height, layout):
    """the [H, W, 3] / [3, H, W] view of one image of a mixed RGB buffer (numpy array or torch tensor of bytes)"""
    row_stride = int(row_stride) or (width if _rgb_layout(layout) == 1 else 3 * width)
    if _rgb_layout(layout) == 1:
        shape, strides = (3, height, width), (row_stride * height, row_stride, 1)
    else:
        shape, strides = (height, width, 3), (row_stride, 3, 1)
    if hasattr(buf, "as_strided"):   # torch
        return buf.as_strided(shape, strides, int(offset))
    return np.lib.stride_tricks.as_strided(buf[int(offset):], shape, strides)


def _size_array(v, n):
    if v is None or isinstance(v, C.Array):
        return v
    return (C.c_size_t * n)(*[int(x) for x in v])


def jpeg_scaled_info(info, scale_denom):
    """the info of a file decoded at 1 / scale_denom (hvc_jpeg_scaled_info): sizes ceil(x * N / 8), tight scaled planes"""
    out = JpegInfo()
    _chk(lib().hvc_jpeg_scaled_info(C.byref(info), scale_denom, C.byref(out)), "hvc_jpeg_scaled_info")
    return out


def jpeg_entropy_decode(data: bytes, info=None, restart_markers=False):
    """Huffman + DC prediction of one frame -> (info, int16 coefficient record).  restart_markers: the extension
    hvc_jpeg_entropy_decode_restart (DRI / RSTn honoured; off = the model's behaviour)"""
    info = info or jpeg_read_header(data)
    coefs = np.empty(info.coef_count, dtype=np.int16)
    fn = "hvc_jpeg_entropy_decode_restart" if restart_markers else "hvc_jpeg_entropy_decode"
    _chk(getattr(lib(), fn)(data, len(data), C.byref(info), coefs.ctypes.data), fn)
    return info, coefs


def jpeg_entropy_decode2(data_a: bytes, data_b: bytes):
    """hvc_jpeg_entropy_decode2: two files decoded in turn on this thread -> ((status, info, record), (status, info, record))"""
    ia, ib = jpeg_read_header(data_a), jpeg_read_header(data_b)
    ca, cb = np.empty(ia.coef_count, dtype=np.int16), np.empty(ib.coef_count, dtype=np.int16)
    sa, sb = C.c_int(1), C.c_int(1)
    _chk(lib().hvc_jpeg_entropy_decode2(data_a, len(data_a), C.byref(ia), ca.ctypes.data, C.byref(sa),
                                        data_b, len(data_b), C.byref(ib), cb.ctypes.data, C.byref(sb)), "hvc_jpeg_entropy_decode2")
    return (sa.value, ia, ca), (sb.value, ib, cb)


def jpeg_get_yuv_frame(info, pixels):
    """Decoder.get_yuv_frame: the crops of components 0, 1, 2 back to back -- HvcError(HVC_E_BAD_JPEG) where the model's
    Frame.of_planes raises (fewer than three components, planes it cannot name as 4:2:0 / 4:2:2 / 4:4:4)."""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    need = sum(info.comp[i].actual_width * info.comp[i].actual_height for i in range(min(info.n_comp, 3)))
    out = np.empty(need, dtype=np.uint8)
    n = C.c_size_t()
    _chk(lib().hvc_jpeg_get_yuv_frame(C.byref(info), pixels.ctypes.data, out.ctypes.data, need, C.byref(n)))
    return out[:n.value]


def jpeg_get_cropped_planes(info, pixels):
    """Decoder.crop over every decoded plane, back to back in scan order, whatever the sampling."""
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    need = sum(info.comp[i].actual_width * info.comp[i].actual_height for i in range(info.n_comp))
    out = np.empty(need, dtype=np.uint8)
    n = C.c_size_t()
    _chk(lib().hvc_jpeg_get_cropped_planes(C.byref(info), pixels.ctypes.data, out.ctypes.data, need, C.byref(n)))
    return out


YUV_FORMATS = {"420": 420, "422": 422, "444": 444, "YUY2": 1, "UYVY": 2, "YVYU": 3}   # Yuv_format.arg_type (yuv_format.ml:66-77)


def yuv_frame_bytes(fmt, width, height):
    n = C.c_size_t()
    _chk(lib().hvc_yuv_frame_bytes(fmt, width, height, C.byref(n)), "hvc_yuv_frame_bytes")
    return n.value


def quant_table(chroma_table, quality):
    out = np.empty(64, dtype=np.uint16)
    _chk(lib().hvc_quant_table(1 if chroma_table else 0, quality, out.ctypes.data))
    return out


def compare_planes(a, b):
    """Ocompare.{max_difference, total_difference, square_error} (tools/src/ocompare.ml:6-47)"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    if a.shape != b.shape:
        raise ValueError("planes differ in size")  # the model asserts (ocompare.ml:9-10)
    mx, tot, se = C.c_int(), C.c_uint64(), C.c_uint64()
    _chk(lib().hvc_compare_planes(a.ctypes.data, b.ctypes.data, a.size, C.byref(mx), C.byref(tot), C.byref(se)))
    return mx.value, tot.value, se.value


def huffman_code_tables(table_set, ctx=None):
    """hvc_huffman_code_tables: the encoder back ends' code tables as {"dc": [[length, bits, category]], "ac": [[[length, bits,
    run, size]]]} -- the shape of tests/golden/g8_code_tables.json (Tables.Encoder.dc_table / ac_table).  ctx = None: the host
    coder's; a Context: the GPU coder's, read back from its device memory."""
    codes = np.zeros(16 + 256, dtype=np.uint32)
    _chk(lib().hvc_huffman_code_tables(ctx._h if ctx is not None else None, table_set, HVC_MEM_DEVICE if ctx is not None else HVC_MEM_HOST,
                                       codes.ctypes.data), "hvc_huffman_code_tables")
    dc = [[int(codes[i]) & 31, int(codes[i]) >> 5, i] for i in range(16) if codes[i]]
    ac = []
    for run in range(16):
        row = [[int(codes[16 + (run << 4 | size)]) & 31, int(codes[16 + (run << 4 | size)]) >> 5, run, size] for size in range(16)]
        while row and row[-1][0] == 0:
            row.pop()
        if row and row[0][0] == 0:     # no size-0 symbol for this run: the model's placeholder (tables.ml:536-543)
            row[0] = [0, 0, 0, 0]
        ac.append(row)
    return {"dc": dc, "ac": ac}


def jpeg_header(info, specs=None, restart_interval=0):
    """SOI .. SOS of the file Encoder.write_headers produces for this geometry / quality; specs: four (bits, vals) pairs
    or HuffSpec (DC0, DC1, AC0, AC1) for the DHT bodies in place of the default tables (hvc_jpeg_header_tables);
    restart_interval: with the DRI segment of that many MCUs in front of SOS (hvc_jpeg_header_restart)"""
    n = C.c_size_t()
    buf = np.empty(4096, dtype=np.uint8)
    if restart_interval:
        _chk(lib().hvc_jpeg_header_restart(C.byref(info), None if specs is None else huff_specs(specs), int(restart_interval),
                                           buf.ctypes.data, buf.size, C.byref(n)), "hvc_jpeg_header_restart")
    elif specs is None:
        _chk(lib().hvc_jpeg_header(C.byref(info), buf.ctypes.data, buf.size, C.byref(n)), "hvc_jpeg_header")
    else:
        _chk(lib().hvc_jpeg_header_tables(C.byref(info), huff_specs(specs), buf.ctypes.data, buf.size, C.byref(n)),
             "hvc_jpeg_header_tables")
    return buf[:n.value].tobytes()


def huffman_spec_from_counts(counts):
    """ITU-T T.81 Annex K.2 over 256 symbol counts (hvc_huffman_spec_from_counts) -> (bits as a list of 16, huffval)"""
    c = np.zeros(256, dtype=np.uint64)
    c[:len(counts)] = np.asarray(counts, dtype=np.uint64)
    s = HuffSpec()
    _chk(lib().hvc_huffman_spec_from_counts(c.ctypes.data, C.byref(s)), "hvc_huffman_spec_from_counts")
    return s.to_pair()


def huffman_optimal_tables(info, coefs, restart_interval=0):
    """the four optimal tables of one frame's coefficient record (hvc_huffman_optimal_tables): [(bits, vals)] DC0, DC1,
    AC0, AC1; restart_interval: over the symbols of the scan cut every so many MCUs (hvc_huffman_optimal_tables_restart)"""
    coefs = np.ascontiguousarray(coefs, dtype=np.int16)
    assert coefs.size >= info.coef_count
    out = (HuffSpec * 4)()
    if restart_interval:
        _chk(lib().hvc_huffman_optimal_tables_restart(C.byref(info), coefs.ctypes.data, int(restart_interval), out),
             "hvc_huffman_optimal_tables_restart")
    else:
        _chk(lib().hvc_huffman_optimal_tables(C.byref(info), coefs.ctypes.data, out), "hvc_huffman_optimal_tables")
    return [s.to_pair() for s in out]


def jpeg_encoder_layout(width, height, chroma, quality):
    info = JpegInfo()
    _chk(lib().hvc_jpeg_encoder_layout(width, height, chroma, quality, C.byref(info)), "hvc_jpeg_encoder_layout")
    return info


class EncoderMixedLayout:
    """what hvc_jpeg_encoder_mixed_layout makes of a list of (width, height, chroma, quality): infos (ctypes array of JpegInfo),
    status (per frame: what jpeg_encoder_layout + hvc_jpeg_encoder_check answer), pixel_offsets (bytes) and coef_offsets (int16
    elements) of the good frames' records, pixel_total and coef_total"""

    def __init__(self, frames, align=0):
        cols = self._columns(frames, ("pixel_offsets", "coef_offsets"))
        pt, ct = C.c_size_t(), C.c_size_t()
        _chk(lib().hvc_jpeg_encoder_mixed_layout(*cols, self.n, align, self.infos, self.status, self.pixel_offsets,
                                                 self.coef_offsets, C.byref(pt), C.byref(ct)), "hvc_jpeg_encoder_mixed_layout")
        self.pixel_total, self.coef_total = pt.value, ct.value

    def _columns(self, frames, arrays):
        """widths, heights, chromas, qualities of `frames` as int arrays; sets n, infos, status and the size_t `arrays`, every
        array max(n, 1) long"""
        self.n = len(frames)
        m = max(self.n, 1)
        self.infos = (JpegInfo * m)()
        self.status = (C.c_int * m)()
        for a in arrays:
            setattr(self, a, (C.c_size_t * m)())
        return [(C.c_int * m)(*[int(f[k]) for f in frames]) for k in range(4)]

    def __len__(self):
        return self.n


def jpeg_encoder_mixed_layout(frames, align=0):
    """frames: (width, height, chroma, quality) each -> EncoderMixedLayout"""
    return EncoderMixedLayout(frames, align)


class EncoderMixedRgbLayout(EncoderMixedLayout):
    """what hvc_jpeg_encoder_mixed_rgb_layout makes of a list of (width, height, chroma, quality): EncoderMixedLayout's members
    (status with the even-size rule of hvc_jpeg_encode_rgb on top), and where every good frame's RGB image goes: rgb_offsets,
    rgb_row_strides, total_bytes (rgb_total), for one `layout` ("interleaved" / "planar")"""

    def __init__(self, frames, layout="interleaved", align=0, row_align=0):
        cols = self._columns(frames, ("rgb_offsets", "rgb_row_strides", "pixel_offsets", "coef_offsets"))
        self.layout = _rgb_layout(layout)
        rt, pt, ct = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _chk(lib().hvc_jpeg_encoder_mixed_rgb_layout(*cols, self.n, self.layout, align, row_align, self.infos, self.status,
                                                     self.rgb_offsets, self.rgb_row_strides, C.byref(rt), self.pixel_offsets,
                                                     self.coef_offsets, C.byref(pt), C.byref(ct)),
             "hvc_jpeg_encoder_mixed_rgb_layout")
        self.total_bytes = self.rgb_total = rt.value
        self.pixel_total, self.coef_total = pt.value, ct.value


def jpeg_encoder_mixed_rgb_layout(frames, layout="interleaved", align=0, row_align=0):
    """frames: (width, height, chroma, quality) each -> EncoderMixedRgbLayout"""
    return EncoderMixedRgbLayout(frames, layout, align, row_align)


def encoder_pixel_record(info, y, u, v, width, height, chroma):
    """the padded pixel record hvc_jpeg_encode hands its block stage (Plane.blit_available of the frame's planes into
    zero-filled planes of jpeg_encoder_layout's geometry, encoder.ml:514-516) -> uint8 array of info.pixel_bytes"""
    out = np.zeros(info.pixel_bytes, dtype=np.uint8)
    cw = width if chroma == 444 else width // 2
    ch = height // 2 if chroma == 420 else height
    for k, (p, sw, sh) in enumerate(((y, width, height), (u, cw, ch), (v, cw, ch))):
        L = info.layout[k]
        bw, bh = min(sw, info.comp[k].decoded_width), min(sh, info.comp[k].decoded_height)
        plane = out[L.plane_offset:L.plane_offset + L.stride * L.blocks_h * 8].reshape(-1, L.stride)
        plane[:bh, :bw] = np.asarray(p, dtype=np.uint8).reshape(sh, sw)[:bh, :bw]
    return out


def restart_slack(info, restart_interval):
    """bytes a restart interval adds to a file at most: 3 per interval (pad byte + marker) and the 6 of DRI"""
    c0 = info.comp[0]
    return _interval_slack((c0.decoded_width // (8 * max(c0.hscale, 1))) * (c0.decoded_height // (8 * max(c0.vscale, 1))),
                           restart_interval)


def _interval_slack(mcus, restart_interval):
    return 3 * -(-mcus // int(restart_interval)) + 6 if restart_interval else 0


def jpeg_entropy_encode(info, coefs, specs=None, restart_interval=0):
    """the whole file of one coefficient record; specs: four (bits, vals) pairs or HuffSpec (DC0, DC1, AC0, AC1) in place
    of the default tables (hvc_jpeg_entropy_encode_tables), "optimised" for the record's own optimal ones;
    restart_interval: DRI + an RSTn marker every so many MCUs (hvc_jpeg_entropy_encode_restart)"""
    coefs = np.ascontiguousarray(coefs, dtype=np.int16)
    assert coefs.size == info.coef_count
    cap = 8 * coefs.size + 4096 + restart_slack(info, restart_interval)  # 26 bits per coefficient at worst, every byte stuffed
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t()
    if restart_interval:
        if isinstance(specs, str) and specs == "optimised":
            specs = huffman_optimal_tables(info, coefs, restart_interval)
        _chk(lib().hvc_jpeg_entropy_encode_restart(C.byref(info), None if specs is None else huff_specs(specs),
                                                   int(restart_interval), coefs.ctypes.data, out.ctypes.data, cap, C.byref(n)),
             "hvc_jpeg_entropy_encode_restart")
    elif specs is None:
        _chk(lib().hvc_jpeg_entropy_encode(C.byref(info), coefs.ctypes.data, out.ctypes.data, cap, C.byref(n)),
             "hvc_jpeg_entropy_encode")
    else:
        if isinstance(specs, str) and specs == "optimised":
            specs = huffman_optimal_tables(info, coefs)
        _chk(lib().hvc_jpeg_entropy_encode_tables(C.byref(info), huff_specs(specs), coefs.ctypes.data, out.ctypes.data, cap,
                                                  C.byref(n)), "hvc_jpeg_entropy_encode_tables")
    return out[:n.value].tobytes()


class Context:
    """hvc_ctx: one per GPU / host thread."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _chk(lib().hvc_create(C.byref(self._h), device), "hvc_create(device=%d)" % device)

    def close(self):
        if self._h:
            lib().hvc_destroy(self._h)   # (drains what is in flight: only then may a submission's buffers go)
            self._h = C.c_void_p()
            getattr(self, "_slot_buffers", {}).clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, handle):
        """handle: a hipStream_t as int, e.g. torch.cuda.current_stream().cuda_stream; 0 = HIP's
        default (null) stream -- which is what PyTorch's default stream is."""
        _chk(lib().hvc_set_stream(self._h, C.c_void_p(handle)))

    def reset_stream(self):
        """back to the context's own (non-blocking) stream"""
        _chk(lib().hvc_reset_stream(self._h))

    def synchronize(self):
        _chk(lib().hvc_synchronize(self._h))

    def set_host_cpus(self, cpulist):
        """which CPUs the batch pipelines' host threads may run on: "0-15,32-47", "auto" (the GPU's NUMA node), None"""
        _chk(lib().hvc_set_host_cpus(self._h, cpulist.encode() if cpulist else None), "hvc_set_host_cpus(%r)" % (cpulist,))

    def get_host_cpus(self):
        buf, n = C.create_string_buffer(256), C.c_int()
        _chk(lib().hvc_get_host_cpus(self._h, buf, 256, C.byref(n)))
        return buf.value.decode(), n.value

    def host_threads(self):
        """(threads the context's pool holds, threads it has ever started): the batch pipelines reuse them"""
        alive, ever = C.c_int(), C.c_uint64()
        _chk(lib().hvc_host_threads(self._h, C.byref(alive), C.byref(ever)))
        return alive.value, ever.value

    def timer_begin(self):
        _chk(lib().hvc_timer_begin(self._h))

    def timer_end(self):
        ms = C.c_float()
        _chk(lib().hvc_timer_end(self._h, C.byref(ms)))
        return ms.value

    def set_restart_markers(self, honour=True):
        """the extension: the context's file-level entry points honour DRI / RSTn (default off = the model's behaviour)"""
        _chk(lib().hvc_set_restart_markers(self._h, 1 if honour else 0), "hvc_set_restart_markers")

    def _set(self, name, table, v):
        """hvc_set_*(ctx, a name of `table` or the number itself)"""
        _chk(getattr(lib(), name)(self._h, _enum(table, v)), name)

    def _get(self, name, start=0):
        """hvc_get_*(ctx, &int) -> the int"""
        v = C.c_int(start)
        _chk(getattr(lib(), name)(self._h, C.byref(v)), name)
        return v.value

    def set_arithmetic(self, arith):
        """"model" (default: the OCaml model's decoder) | "hardcaml" (the reference's RTL decoder datapath, bit for bit) |
        "libjpeg" (libjpeg's islow inverse DCT and, in the RGB forms, its fancy upsampling, bit for bit): the block stage
        of every decode entry point except the fused 4:4:4, scaled and mixed ones, which refuse anything but "model"."""
        self._set("hvc_set_arithmetic", HVC_ARITH, arith)

    @property
    def arithmetic(self):
        v = self._get("hvc_get_arithmetic")
        return ARITH_NAMES.get(v, v)

    def set_mixed_arithmetic(self, arith):
        """hvc_set_mixed_arithmetic: "model" (default) | "libjpeg" -- the mixed decode calls' own setting.  Under "libjpeg"
        decode_frames_mixed, yuv_to_rgb_mixed, decode_frames_mixed_rgb, jpeg_decode_batch_mixed, _mixed_rgb and _mixed_resized
        at full size give libjpeg's pixels (what jpeg_decode / jpeg_decode_rgb give per file under set_arithmetic("libjpeg"))
        whatever set_arithmetic says, and the reduced-size forms are refused.  Anything else ("hardcaml" included) is an error
        and leaves the setting as it was."""
        self._set("hvc_set_mixed_arithmetic", HVC_ARITH, arith)

    @property
    def mixed_arithmetic(self):
        v = self._get("hvc_get_mixed_arithmetic")
        return ARITH_NAMES.get(v, v)

    def decode_divergence(self, coefs, coef_frame_stride, qtabs, comps, n_frames, max_diff=None, diff_frame_stride=None):
        """max |model - hardcaml| per block (hvc_decode_frames_divergence) -> uint8 array [n_frames, blocks per frame]
        (host records), or into max_diff (device records: a torch uint8 tensor of n_frames * diff_frame_stride)"""
        ca, w1 = _addr(coefs)
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(-1, 64)
        arr = comps if not isinstance(comps, list) else components(comps)
        blocks = sum(a.blocks_w * a.blocks_h for a in arr)
        stride = blocks if diff_frame_stride is None else diff_frame_stride
        if max_diff is None:
            assert w1 == HVC_MEM_HOST, "device records: pass a device max_diff"
            max_diff = np.zeros((n_frames, stride), dtype=np.uint8)
        da, w2 = _addr(max_diff)
        assert w1 == w2
        _chk(lib().hvc_decode_frames_divergence(self._h, ca, coef_frame_stride, q.ctypes.data, q.shape[0], arr, len(arr),
                                                n_frames, da, stride, w1), "hvc_decode_frames_divergence")
        return max_diff

    def dct_fixed(self, direction, rom_prec, transpose_prec, blocks, out=None):
        """Fixed_point.forward_transform / inverse_transform of int32 blocks [n, 8, 8] (hvc_dct_fixed): a numpy array, or a
        torch device tensor with a device `out`.  direction "forward" | "inverse" (or 0 | 1)."""
        ia, w1 = _addr(blocks)
        if out is None:
            assert w1 == HVC_MEM_HOST, "device blocks: pass a device out"
            out = np.zeros(np.shape(blocks), dtype=np.int32)
        oa, w2 = _addr(out)
        assert w1 == w2
        n = int(np.prod(tuple(blocks.shape))) // 64
        _chk(lib().hvc_dct_fixed(self._h, _dct_direction(direction), int(rom_prec), int(transpose_prec), ia, oa, n, w1),
             "hvc_dct_fixed")
        return out

    def dct_reference(self, direction, blocks, out=None):
        """the float64 reference transform of int32 blocks [n, 8, 8] (hvc_dct_reference) -> float64, as dct_fixed"""
        ia, w1 = _addr(blocks)
        if out is None:
            assert w1 == HVC_MEM_HOST, "device blocks: pass a device out"
            out = np.zeros(np.shape(blocks), dtype=np.float64)
        oa, w2 = _addr(out)
        assert w1 == w2
        n = int(np.prod(tuple(blocks.shape))) // 64
        _chk(lib().hvc_dct_reference(self._h, _dct_direction(direction), ia, oa, n, w1), "hvc_dct_reference")
        return out

    def dct_error_search(self, cfgs, seed, range_, first_block, n_blocks):
        """generated blocks first_block .. + n_blocks through every configuration (hvc_dct_error_search): cfgs as
        dct_configs takes them -> (max_error float64 [n_cfg], worst_block uint64 [n_cfg])"""
        arr = cfgs if isinstance(cfgs, C.Array) else dct_configs(cfgs)
        res = (DctError * len(arr))()
        _chk(lib().hvc_dct_error_search(self._h, arr, len(arr), int(seed), int(range_), int(first_block), int(n_blocks),
                                        res), "hvc_dct_error_search")
        return (np.array([r.max_error for r in res], dtype=np.float64),
                np.array([r.worst_block for r in res], dtype=np.uint64))

    def set_encode_arithmetic(self, arith):
        """"model" (default: the OCaml model's encoder) | "hardcaml" (the reference's RTL encoder DCT and quantiser, bit
        for bit): the block stage of every encode entry point.  Independent of set_arithmetic."""
        self._set("hvc_set_encode_arithmetic", HVC_ARITH, arith)

    @property
    def encode_arithmetic(self):
        v = self._get("hvc_get_encode_arithmetic")
        return ARITH_NAMES.get(v, v)

    def set_encode_libjpeg(self, on=True):
        """hvc_set_encode_libjpeg: the encoder bit-exact to libjpeg-turbo (jfdctint.c's forward DCT, its rounded division,
        replicated edges and dummy blocks; from RGB its biased chroma averaging) for fdct_quant, encode_frames,
        encode_frames_submit, jpeg_encode, jpeg_encode_batch, rgb_to_yuv, jpeg_encode_rgb and the mixed encode calls, from planes
        and from RGB, with either coder.  A setting of its own: set_encode_arithmetic is then not consulted, except that
        "hardcaml" beside it is refused at the encode call.  encode_frames_recon and encode_divergence have no libjpeg form and
        are refused under it."""
        _chk(lib().hvc_set_encode_libjpeg(self._h, int(on) if isinstance(on, (bool, np.bool_)) else on), "hvc_set_encode_libjpeg")

    @property
    def encode_libjpeg(self):
        return bool(self._get("hvc_get_encode_libjpeg"))

    def set_huffman_tables(self, which):
        """"default" (the Annex K tables, every byte as before) | "optimised" (each file's own Annex K.2 tables): the files of
        jpeg_encode and jpeg_encode_batch (both coders).  Independent of set_encode_arithmetic."""
        self._set("hvc_set_huffman_tables", HVC_HUFF, which)

    def set_restart_interval(self, mcus):
        """0 (default: no DRI, no RSTn, every byte as before) | 1 .. 65535: the files of jpeg_encode and jpeg_encode_batch
        (both coders) carry a DRI segment and an RSTn marker every `mcus` MCUs.  Independent of set_huffman_tables,
        set_encode_arithmetic and the reader's set_restart_markers."""
        _chk(lib().hvc_set_restart_interval(self._h, int(mcus)), "hvc_set_restart_interval")

    @property
    def restart_interval(self):
        return self._get("hvc_get_restart_interval")

    @property
    def huffman_tables(self):
        v = self._get("hvc_get_huffman_tables")
        return HUFF_NAMES.get(v, v)

    def encode_divergence(self, pixels, pixel_frame_stride, qtabs, comps, n_frames, max_diff=None, diff_frame_stride=None):
        """min(255, max |q_model - q_hardcaml|) per block (hvc_encode_frames_divergence) -> uint8 array [n_frames, blocks
        per frame] (host pixels), or into max_diff (device pixels: a torch uint8 tensor of n_frames * diff_frame_stride)"""
        pa, w1 = _addr(pixels)
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(-1, 64)
        arr = comps if not isinstance(comps, list) else components(comps)
        blocks = sum(a.blocks_w * a.blocks_h for a in arr)
        stride = blocks if diff_frame_stride is None else diff_frame_stride
        if max_diff is None:
            assert w1 == HVC_MEM_HOST, "device pixels: pass a device max_diff"
            max_diff = np.zeros((n_frames, stride), dtype=np.uint8)
        da, w2 = _addr(max_diff)
        assert w1 == w2
        _chk(lib().hvc_encode_frames_divergence(self._h, pa, pixel_frame_stride, q.ctypes.data, q.shape[0], arr, len(arr),
                                                n_frames, da, stride, w1), "hvc_encode_frames_divergence")
        return max_diff

    def set_decode_kernel(self, which):
        """0 packed (default) | 1 unpacked int32 | 2 int64 for every block -- identical output"""
        _chk(lib().hvc_set_decode_kernel(self._h, which))

    def set_profiling(self, on=True):
        _chk(lib().hvc_set_profiling(self._h, 1 if on else 0))

    def last_kernel_ms(self):
        ms = C.c_float()
        _chk(lib().hvc_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def kernel_ms_history(self, n):
        arr = (C.c_float * n)()
        _chk(lib().hvc_kernel_ms_history(self._h, arr, n))
        return list(arr)

    def checksum_records(self, data, record_bytes, n_records, record_stride=None):
        """K5: position-weighted 64-bit checksum per record (numpy uint64 array); data: numpy (host) or a
        device tensor / address."""
        a, where = _addr(data)
        sums = np.zeros(max(n_records, 1), dtype=np.uint64)
        _chk(lib().hvc_checksum_records(self._h, a, record_bytes, record_bytes if record_stride is None else record_stride,
                                        n_records, sums.ctypes.data, where), "hvc_checksum_records")
        return sums[:n_records]

    def last_wide_blocks(self):
        n = C.c_uint64()
        _chk(lib().hvc_last_wide_blocks(self._h, C.byref(n)))
        return n.value

    # -- the asynchronous seam: pinned host memory + slots ---------------------
    def host_alloc(self, shape, dtype=np.uint8):
        """pinned host memory (hvc_host_alloc) as a numpy array; give it back with host_free(array)"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        _chk(lib().hvc_host_alloc(self._h, n, C.byref(p)), "hvc_host_alloc(%d)" % n)
        buf = (C.c_uint8 * max(n, 1)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def host_free(self, arr):
        _chk(lib().hvc_host_free(self._h, arr.ctypes.data), "hvc_host_free")

    def host_register(self, arr):
        """pins memory the caller owns in place; host_unregister(arr) before it goes.  Whole pages only (include/hvc_jpeg.h):
        arr from page_aligned_empty(), whose allocation is registered to its last page"""
        size = (arr.nbytes + PAGE - 1) // PAGE * PAGE
        _chk(lib().hvc_host_register(self._h, arr.ctypes.data, size), "hvc_host_register")

    def host_unregister(self, arr):
        _chk(lib().hvc_host_unregister(self._h, arr.ctypes.data), "hvc_host_unregister")

    def decode_frames_submit(self, slot, coefs, coef_frame_stride, qtabs, comps, n_frames, pixels, pixel_frame_stride):
        """hvc_decode_frames on HOST coefficient records (numpy; pinned for the overlap), asynchronously in `slot`;
        pixels: numpy (host: downloaded) or a device tensor / address (written in place).  wait(slot) completes it."""
        ca, w1 = _addr(coefs)
        assert w1 == HVC_MEM_HOST, "the coefficient records of a submission are host memory"
        pa, w2 = _addr(pixels)
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(-1, 64)
        arr = comps if not isinstance(comps, list) else components(comps)
        _chk(lib().hvc_decode_frames_submit(self._h, slot, ca, coef_frame_stride, q.ctypes.data, q.shape[0], arr, len(arr),
                                            n_frames, pa, pixel_frame_stride, w2), "hvc_decode_frames_submit(slot %d)" % slot)
        self._keep(slot, coefs, pixels)

    def encode_frames_submit(self, slot, pixels, pixel_frame_stride, qtabs, comps, n_frames, coefs, coef_frame_stride):
        """the encoder mirror: HOST pixel records in, coefficient records to numpy (host) or a device tensor"""
        pa, w1 = _addr(pixels)
        assert w1 == HVC_MEM_HOST, "the pixel records of a submission are host memory"
        ca, w2 = _addr(coefs)
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(-1, 64)
        arr = comps if not isinstance(comps, list) else components(comps)
        _chk(lib().hvc_encode_frames_submit(self._h, slot, pa, pixel_frame_stride, q.ctypes.data, q.shape[0], arr, len(arr),
                                            n_frames, ca, coef_frame_stride, w2), "hvc_encode_frames_submit(slot %d)" % slot)
        self._keep(slot, pixels, coefs)

    def _keep(self, slot, *buffers):
        """the ABI's rule: a submission's buffers stay valid until its hvc_wait -- an upload from memory the interpreter has
        meanwhile freed is a GPU page fault (tools/stress_seam.py found it the hard way), so the binding holds on to them"""
        if not hasattr(self, "_slot_buffers"):
            self._slot_buffers = {}
        self._slot_buffers[slot] = buffers

    def wait(self, slot):
        try:
            _chk(lib().hvc_wait(self._h, slot), "hvc_wait(slot %d)" % slot)
        finally:
            getattr(self, "_slot_buffers", {}).pop(slot, None)

    def slot_done(self, slot):
        d = C.c_int()
        _chk(lib().hvc_slot_query(self._h, slot, C.byref(d)), "hvc_slot_query")
        return bool(d.value)

    def slot_last_stats(self, slot):
        st = SlotStats()
        _chk(lib().hvc_slot_last_stats(self._h, slot, C.byref(st)), "hvc_slot_last_stats")
        return st

    # -- decode -------------------------------------------------------------
    def dequant_idct_recon(self, coefs, qtab, blocks_w, blocks_h, n_planes, plane, stride=None,
                           coef_plane_stride=0, plane_stride=0):
        ca, pa, w1 = _same_space(coefs, "coefs", plane, "plane")
        q = np.ascontiguousarray(qtab, dtype=np.uint16)
        assert q.size == 64
        _chk(lib().hvc_dequant_idct_recon(self._h, ca, coef_plane_stride, q.ctypes.data, blocks_w, blocks_h,
                                          n_planes, pa, stride or blocks_w * 8, plane_stride, w1))

    def decode_frames(self, coefs, coef_frame_stride, qtabs, comps, n_frames, pixels, pixel_frame_stride):
        ca, w1 = _addr(coefs)
        pa, w2 = _addr(pixels)
        assert w1 == w2
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(-1, 64)
        arr = comps if not isinstance(comps, list) else components(comps)
        _chk(lib().hvc_decode_frames(self._h, ca, coef_frame_stride, q.ctypes.data, q.shape[0], arr, len(arr),
                                     n_frames, pa, pixel_frame_stride, w1))

    def decode_frames_mixed(self, coefs, coef_offsets, infos, pixels, pixel_offsets):
        """hvc_decode_frames_mixed: frame f = infos[f] (JpegInfo: layout and tables), its coefficient record at
        coefs[coef_offsets[f]:] (int16 elements), its pixel record at pixels[pixel_offsets[f]:] (bytes).  coefs / pixels:
        numpy (host) or torch cuda tensors, both in the same memory space."""
        ca, pa, w1 = _same_space(coefs, "coefs", pixels, "pixels")
        n = len(infos)
        _chk(lib().hvc_decode_frames_mixed(self._h, ca, _size_array(coef_offsets, n), _infos_array(infos), n, pa,
                                           _size_array(pixel_offsets, n), w1), "hvc_decode_frames_mixed")

    def _decode_batch_mixed(self, name, lay, buf, device, middle, out_infos, image):
        """the tail of the four mixed batch decode calls: name(ctx, files, n, *middle, infos, status, offsets, buf, capacity,
        [layout,] where, stats) into buf (None: made here, zero-filled, on the device with `device`), the stats into
        self.last_batch_stats, and one (status, info, view) per file -- info = out_infos[f] (lay.infos or lay.scaled), None for a
        file the layout refused; view = the planes of info (a file the layout took), or, with `image`, the RGB image (a file that
        decoded and has a size), else None"""
        n = len(lay)
        if buf is None:
            buf = _zeroed_bytes(lay.total_bytes, device)
        addr, where = _addr(buf)
        st = BatchStats()
        status = (C.c_int * n)(*lay.status)
        tail = (lay.rgb_offsets, lay.rgb_row_strides, addr, _capacity(buf), lay.layout) if image else \
               (lay.pixel_offsets, addr, _capacity(buf))
        _chk(getattr(lib(), name)(self._h, lay.ptrs, lay.sizes, n, *middle, lay.infos, status, *tail, where, C.byref(st)), name)
        self.last_batch_stats = st
        out = []
        for f in range(n):
            info, view = (out_infos[f] if lay.status[f] == 0 else None), None
            if info is not None and not image:
                off = lay.pixel_offsets[f]
                view = info.planes(buf[off:off + info.pixel_bytes])
            elif info is not None and status[f] == 0 and info.width > 0 and info.height > 0:
                view = rgb_view(buf, lay.rgb_offsets[f], lay.rgb_row_strides[f], info.width, info.height, lay.layout)
            out.append((status[f], info, view))
        return out

    def jpeg_decode_batch_mixed(self, jpegs, threads=8, chunk_bytes=0, device=False, layout=None, pixels=None):
        """Files of any sizes, samplings and tables in one call.  Returns one (status, info, planes) per file: status = the file's
        own hvc_status (0 = decoded), planes = info.planes(...) views of ONE buffer (numpy, or a torch cuda tensor with
        device=True), None for a file whose header could not be read.  layout / pixels: a MixedLayout made before and a buffer of
        layout.total_bytes to decode into (default: made here, zero-filled).  The call's hvc_batch_stats: self.last_batch_stats."""
        lay = layout if layout is not None else MixedLayout(jpegs)
        return self._decode_batch_mixed("hvc_jpeg_decode_batch_mixed", lay, pixels, device, (threads, chunk_bytes), lay.infos, False)

    def yuv_to_rgb_mixed(self, yuv, yuv_offsets, infos, rgb, rgb_offsets, rgb_row_strides=None, layout="interleaved"):
        """hvc_yuv_to_rgb_mixed: the colour pass over images of any size and sampling in one launch.  Frame f = infos[f]
        (JpegInfo: width, height, sampling factors, layout), its planes at yuv[yuv_offsets[f]:], its image at
        rgb[rgb_offsets[f]:] with rows rgb_row_strides[f] apart (None: tight).  yuv / rgb: numpy (host) or torch cuda
        tensors of bytes, both in the same memory space."""
        ya, ra, w1 = _same_space(yuv, "yuv", rgb, "rgb")
        n = len(infos)
        _chk(lib().hvc_yuv_to_rgb_mixed(self._h, ya, _size_array(yuv_offsets, n), _infos_array(infos), n, ra, _size_array(rgb_offsets, n),
                                        _size_array(rgb_row_strides, n), _rgb_layout(layout), w1), "hvc_yuv_to_rgb_mixed")

    def rgb_to_yuv_mixed(self, yuv, yuv_offsets, infos, rgb, rgb_offsets, rgb_row_strides=None, layout="interleaved"):
        """hvc_rgb_to_yuv_mixed: the way back of yuv_to_rgb_mixed, argument for argument: frame f's image at rgb[rgb_offsets[f]:]
        is read, its planes at yuv[yuv_offsets[f]:] (laid out by infos[f].layout) are written -- the frame's own samples only.
        Sizes are even where the sampling asks for it (hvc_rgb_to_yuv's rule)."""
        ya, ra, w1 = _same_space(yuv, "yuv", rgb, "rgb")
        n = len(infos)
        _chk(lib().hvc_rgb_to_yuv_mixed(self._h, ya, _size_array(yuv_offsets, n), _infos_array(infos), n, ra, _size_array(rgb_offsets, n),
                                        _size_array(rgb_row_strides, n), _rgb_layout(layout), w1), "hvc_rgb_to_yuv_mixed")

    def encode_frames_mixed_rgb(self, rgb, rgb_offsets, infos, coefs, coef_offsets, rgb_row_strides=None, layout="interleaved"):
        """hvc_encode_frames_mixed_rgb: frame f = infos[f] (JpegInfo), its RGB image at rgb[rgb_offsets[f]:] (bytes, rows
        rgb_row_strides[f] apart, None: tight), its coefficient record written at coefs[coef_offsets[f]:] (int16 elements): the
        mixed colour pass into zeroed padded planes in context scratch, then the mixed block stage.  rgb / coefs: numpy (host)
        or torch cuda tensors, both in the same memory space."""
        ra, ca, w1 = _same_space(rgb, "rgb", coefs, "coefs")
        n = len(infos)
        _chk(lib().hvc_encode_frames_mixed_rgb(self._h, ra, _size_array(rgb_offsets, n), _size_array(rgb_row_strides, n),
                                               _rgb_layout(layout), _infos_array(infos), n, ca, _size_array(coef_offsets, n), w1),
             "hvc_encode_frames_mixed_rgb")

    def decode_frames_mixed_rgb(self, coefs, coef_offsets, infos, rgb, rgb_offsets, rgb_row_strides=None, layout="interleaved"):
        """hvc_decode_frames_mixed_rgb: hvc_decode_frames_mixed into context scratch, then the mixed colour pass; arguments as
        decode_frames_mixed and yuv_to_rgb_mixed."""
        ca, ra, w1 = _same_space(coefs, "coefs", rgb, "rgb")
        n = len(infos)
        _chk(lib().hvc_decode_frames_mixed_rgb(self._h, ca, _size_array(coef_offsets, n), _infos_array(infos), n, ra, _size_array(rgb_offsets, n),
                                               _size_array(rgb_row_strides, n), _rgb_layout(layout), w1), "hvc_decode_frames_mixed_rgb")

    def jpeg_decode_batch_mixed_rgb(self, jpegs, threads=8, chunk_bytes=0, device=False, layout="interleaved", row_align=0,
                                    rgb_layout=None, rgb=None):
        """Files of any sizes, samplings and tables to RGB images in one call.  Returns one (status, info, image) per file:
        status = the file's own hvc_status (0 = decoded), image = a [H, W, 3] (interleaved) or [3, H, W] (planar) view into ONE
        buffer (numpy, or a torch cuda tensor with device=True), None for a file that failed.  rgb_layout / rgb: a
        MixedRgbLayout made before and a buffer of rgb_layout.total_bytes to decode into (default: made here, zero-filled).
        The call's hvc_batch_stats: self.last_batch_stats."""
        lay = rgb_layout if rgb_layout is not None else MixedRgbLayout(jpegs, layout, 0, row_align)
        return self._decode_batch_mixed("hvc_jpeg_decode_batch_mixed_rgb", lay, rgb, device, (threads, chunk_bytes), lay.infos, True)

    def decode_frames_mixed_scaled(self, coefs, coef_offsets, infos, scale_denom, pixels, pixel_offsets):
        """hvc_decode_frames_mixed_scaled: decode_frames_mixed at 1 / scale_denom; infos[f].layout's plane_offset / stride place
        planes of blocks_w * N x blocks_h * N samples, N = 8 / scale_denom (any offset, any stride >= blocks_w * N)."""
        ca, pa, w1 = _same_space(coefs, "coefs", pixels, "pixels")
        n = len(infos)
        _chk(lib().hvc_decode_frames_mixed_scaled(self._h, ca, _size_array(coef_offsets, n), _infos_array(infos), n, scale_denom, pa,
                                                  _size_array(pixel_offsets, n), w1), "hvc_decode_frames_mixed_scaled")

    def jpeg_decode_batch_mixed_scaled(self, jpegs, scale_denom, threads=8, chunk_bytes=0, device=False, layout=None, pixels=None):
        """Files of any sizes, samplings and tables at 1 / scale_denom in one call.  Returns one (status, scaled info, planes) per
        file, as jpeg_decode_batch_mixed does at full size; planes = views of the scaled padded planes inside ONE buffer.
        layout / pixels: a MixedScaledLayout made before and a buffer of layout.total_bytes (default: made here, zero-filled)."""
        lay = layout if layout is not None else MixedScaledLayout(jpegs, scale_denom)
        return self._decode_batch_mixed("hvc_jpeg_decode_batch_mixed_scaled", lay, pixels, device, (threads, chunk_bytes, scale_denom),
                                        lay.scaled, False)

    def jpeg_decode_batch_mixed_scaled_rgb(self, jpegs, scale_denom, threads=8, chunk_bytes=0, device=False, layout="interleaved",
                                           row_align=0, rgb_layout=None, rgb=None):
        """Files of any sizes, samplings and tables to RGB images at 1 / scale_denom in one call.  Returns one (status, scaled
        info, image) per file, as jpeg_decode_batch_mixed_rgb does at full size.  rgb_layout / rgb: a MixedScaledRgbLayout made
        before and a buffer of rgb_layout.total_bytes (default: made here, zero-filled)."""
        lay = rgb_layout if rgb_layout is not None else MixedScaledRgbLayout(jpegs, scale_denom, layout, 0, row_align)
        return self._decode_batch_mixed("hvc_jpeg_decode_batch_mixed_scaled_rgb", lay, rgb, device, (threads, chunk_bytes, scale_denom),
                                        lay.scaled, True)

    def rgb_resize_mixed(self, src, src_offsets, widths, heights, dst, dst_offsets, out_widths, out_heights, filter="bilinear",
                         layout="interleaved", src_row_strides=None, dst_row_strides=None, boxes=None, mirror=None, dtype=None,
                         mean=None, std=None, lut=None):
        """hvc_rgb_resize_mixed: image i (widths[i] x heights[i] at src[src_offsets[i]:], rows src_row_strides[i] apart, None:
        tight) to out_widths[i] x out_heights[i] at dst[dst_offsets[i]:] (rows dst_row_strides[i] apart), bit-exact to Pillow's
        Image.resize for filter "box" / "bilinear" / "bicubic" (tools/resize_reference.py), one launch per pass for the whole
        set.  src / dst: numpy (host) or torch cuda tensors of bytes, both in the same memory space.
        boxes / mirror / dtype with mean, std / lut (resize_opts): hvc_rgb_resize_mixed_opts -- Pillow's resize(box=...), a
        left-right flip, and elements of dtype looked up in a table instead of bytes; dst offsets and strides stay in BYTES."""
        sa, da, w1 = _same_space(src, "src", dst, "dst")
        n = len(widths)
        ints = lambda v: (C.c_int * max(n, 1))(*[int(x) for x in v])
        opts, keep, _, _ = resize_opts(n, boxes, mirror, dtype, mean, std, lut)
        if opts is not None:
            _chk(lib().hvc_rgb_resize_mixed_opts(self._h, sa, _size_array(src_offsets, n), _size_array(src_row_strides, n),
                                                 ints(widths), ints(heights), n, da, _size_array(dst_offsets, n),
                                                 _size_array(dst_row_strides, n), ints(out_widths), ints(out_heights),
                                                 _rgb_layout(layout), _resize_filter(filter), w1, C.byref(opts)),
                 "hvc_rgb_resize_mixed_opts")
            del keep
            return
        _chk(lib().hvc_rgb_resize_mixed(self._h, sa, _size_array(src_offsets, n), _size_array(src_row_strides, n), ints(widths),
                                        ints(heights), n, da, _size_array(dst_offsets, n), _size_array(dst_row_strides, n),
                                        ints(out_widths), ints(out_heights), _rgb_layout(layout), _resize_filter(filter), w1),
             "hvc_rgb_resize_mixed")

    def jpeg_decode_batch_mixed_resized(self, jpegs, size=None, sizes=None, filter="bilinear", scale_denom=1, layout="interleaved",
                                        device=False, threads=8, chunk_bytes=0, mixed_layout=None, out=None, boxes=None, mirror=None,
                                        dtype=None, mean=None, std=None, lut=None):
        """Files of any sizes, samplings and tables decoded (at 1 / scale_denom), converted to RGB and resized on the GPU in one
        call (hvc_jpeg_decode_batch_mixed_resized).  size=(W, H): every file to W x H; returns (status[], tensor) with tensor
        [n, H, W, 3] (interleaved) or [n, 3, H, W] (planar) -- numpy, or a torch cuda tensor with device=True; the frame of a
        file that failed keeps what `out` held (zeros when it is made here).  sizes=[(W, H), ...]: a size per file (aspect-
        preserving thumbnails); returns (status[], views), one [H, W, 3] / [3, H, W] view into ONE buffer per file, None for a
        file that failed.  mixed_layout: a MixedLayout made before (its headers are what is needed).  out: the buffer to write
        (bytes; uniform: n * H * W * 3).  The call's hvc_batch_stats: self.last_batch_stats.
        boxes / mirror / dtype with mean, std / lut (resize_opts): hvc_jpeg_decode_batch_mixed_resized_opts -- a box per file in
        the coordinates of its image at 1 / scale_denom (RandomResizedCrop, a centre crop), a left-right flip per file, and a
        tensor of dtype ("float32" / "float16" / "bfloat16", or a torch / numpy dtype) normalised per channel as torchvision's
        ToTensor() + Normalize(mean, std), or looked up in a table of the caller's own (lut, [3, 256]); `out` stays a buffer of
        BYTES (elements * itemsize), the tensor returned is a view of it in dtype."""
        assert (size is None) != (sizes is None), "one of size= and sizes="
        lay = mixed_layout if mixed_layout is not None else MixedLayout(jpegs)
        n = len(lay)
        opts, keep, esz, ename = resize_opts(n, boxes, mirror, dtype, mean, std, lut)
        wh = [tuple(int(v) for v in size)] * n if size is not None else [tuple(int(v) for v in s) for s in sizes]
        assert len(wh) == n
        offs, total = (C.c_size_t * max(n, 1))(), 0
        for f, (w, h) in enumerate(wh):
            offs[f] = total
            total += 3 * max(w, 0) * max(h, 0) * esz
        if out is None:
            out = _zeroed_bytes(total, device)
        oa, where = _addr(out)
        cap = _capacity(out)
        st = BatchStats()
        status = (C.c_int * max(n, 1))(*lay.status)
        ow, oh = (C.c_int * max(n, 1))(*[w for w, _ in wh]), (C.c_int * max(n, 1))(*[h for _, h in wh])
        if opts is None:
            _chk(lib().hvc_jpeg_decode_batch_mixed_resized(self._h, lay.ptrs, lay.sizes, n, threads, chunk_bytes, scale_denom, lay.infos,
                                                           status, ow, oh, offs, None, oa, cap, _rgb_layout(layout),
                                                           _resize_filter(filter), where, C.byref(st)),
                 "hvc_jpeg_decode_batch_mixed_resized")
        else:
            _chk(lib().hvc_jpeg_decode_batch_mixed_resized_opts(self._h, lay.ptrs, lay.sizes, n, threads, chunk_bytes, scale_denom,
                                                                lay.infos, status, ow, oh, offs, None, oa, cap, _rgb_layout(layout),
                                                                _resize_filter(filter), where, C.byref(st), C.byref(opts)),
                 "hvc_jpeg_decode_batch_mixed_resized_opts")
        del keep
        self.last_batch_stats = st
        status = [status[f] for f in range(n)]
        if size is not None:
            w, h = wh[0] if n else (int(size[0]), int(size[1]))
            flat = out[:n * 3 * w * h * esz]
            return status, typed_view(flat, ename, esz).reshape((n,) + rgb_shape(layout, w, h))
        if esz > 1:   # views in elements: offsets counted in elements of the typed buffer
            typed = typed_view(out[:total], ename, esz)
            return status, [rgb_view(typed, offs[f] // esz, 0, wh[f][0], wh[f][1], layout) if status[f] == 0 else None for f in range(n)]
        return status, [rgb_view(out, offs[f], 0, wh[f][0], wh[f][1], layout) if status[f] == 0 else None for f in range(n)]

    def decode_frames_yuv444(self, coefs, coef_frame_stride, qtabs, comps, n_frames, width, height, frames,
                             frame_stride=None):
        """4:2:0 coefficient records -> tight 4:4:4 frames (block stage + crop + supersample_hv2 fused)."""
        ca, w1 = _addr(coefs)
        fa, w2 = _addr(frames)
        assert w1 == w2
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(-1, 64)
        arr = comps if not isinstance(comps, list) else components(comps)
        _chk(lib().hvc_decode_frames_yuv444(self._h, ca, coef_frame_stride, q.ctypes.data, q.shape[0], arr, len(arr),
                                            n_frames, width, height, fa,
                                            3 * width * height if frame_stride is None else frame_stride, w1),
             "hvc_decode_frames_yuv444")

    def jpeg_decode(self, data: bytes):
        """Decoder.decode_a_frame minus the crop: (info, padded pixel record as numpy uint8)"""
        info = jpeg_read_header(data)
        pixels = np.zeros(info.pixel_bytes, dtype=np.uint8)
        _chk(lib().hvc_jpeg_decode(self._h, data, len(data), C.byref(info), pixels.ctypes.data, pixels.size),
             "hvc_jpeg_decode")
        return info, pixels

    def jpeg_decode_yuv444(self, data: bytes):
        """decode_a_frame + Planar_444.of_420 for a 4:2:0 file: (info, uint8 [3][height][width])"""
        info = jpeg_read_header(data)
        frame = np.zeros(3 * info.width * info.height, dtype=np.uint8)
        _chk(lib().hvc_jpeg_decode_yuv444(self._h, data, len(data), C.byref(info), frame.ctypes.data, frame.size),
             "hvc_jpeg_decode_yuv444")
        return info, frame.reshape(3, info.height, info.width)

    def jpeg_decode_batch(self, jpegs, pixels, pixel_frame_stride, threads=8, frames_per_chunk=32, yuv444=False,
                          gpu_entropy=False):
        """config 3 pipeline.  jpegs: list of bytes; pixels: numpy (host) or torch cuda tensor.
        yuv444: 4:2:0 files straight to tight 4:4:4 frames (3 * width * height bytes each).
        gpu_entropy: the Huffman reader on the GPU as well (hvc_jpeg_decode_batch_gpu)."""
        n = len(jpegs)
        ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(j), C.c_void_p) for j in jpegs])
        sizes = (C.c_size_t * n)(*[len(j) for j in jpegs])
        pa, where = _addr(pixels)
        st = BatchStats()
        if gpu_entropy:
            _chk(lib().hvc_jpeg_decode_batch_gpu(self._h, ptrs, sizes, n, threads, frames_per_chunk, pa, pixel_frame_stride,
                                                 where, 1 if yuv444 else 0, C.byref(st)), "hvc_jpeg_decode_batch_gpu")
            return st
        fn = lib().hvc_jpeg_decode_batch_yuv444 if yuv444 else lib().hvc_jpeg_decode_batch
        _chk(fn(self._h, ptrs, sizes, n, threads, frames_per_chunk, pa, pixel_frame_stride, where, C.byref(st)),
             "hvc_jpeg_decode_batch_yuv444" if yuv444 else "hvc_jpeg_decode_batch")
        return st

    def jpeg_encode(self, y, u, v, width, height, chroma=420, quality=75):
        """Encoder.encode_420/422/444 ~frame ~quality -> jpeg bytes"""
        y, u, v = (np.ascontiguousarray(p, dtype=np.uint8) for p in (y, u, v))
        cap = 4 * width * height + 65536 + self._restart_slack(width, height)
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t()
        _chk(lib().hvc_jpeg_encode(self._h, y.ctypes.data, u.ctypes.data, v.ctypes.data, width, height, chroma, quality,
                                   out.ctypes.data, cap, C.byref(n)), "hvc_jpeg_encode")
        return out[:n.value].tobytes()

    # -- RGB (JFIF colour conversion fused with the chroma resampling; include/hvc_jpeg.h, RGB) ---------------
    def yuv_to_rgb(self, yuv, comps, sampling, width, height, rgb, chroma_size=None, n_frames=1, yuv_frame_stride=0,
                   layout="interleaved", rgb_row_stride=0, rgb_frame_stride=0):
        """planes that are already there -> RGB (hvc_yuv_to_rgb).  yuv / rgb: numpy arrays or torch CUDA tensors; comps
        place the planes (plane_offset, stride); sampling 420 | 422 | 444 | 400; chroma_size: the valid chroma samples
        (default: the ceil halves the image needs)."""
        ya, w1 = _addr(yuv)
        ra, w2 = _addr(rgb)
        assert w1 == w2
        arr = comps if not isinstance(comps, list) else components(comps)
        cw, ch = chroma_size or rgb_chroma_window(sampling, width, height)
        _chk(lib().hvc_yuv_to_rgb(self._h, ya, yuv_frame_stride, arr, sampling, width, height, cw, ch, n_frames, ra,
                                  rgb_row_stride, rgb_frame_stride, _rgb_layout(layout), w1), "hvc_yuv_to_rgb")

    def rgb_to_yuv(self, rgb, width, height, sampling, yuv, comps, n_frames=1, yuv_frame_stride=0, layout="interleaved",
                   rgb_row_stride=0, rgb_frame_stride=0):
        """RGB -> planes at the offsets and strides of comps (hvc_rgb_to_yuv); only the frame's own samples are written"""
        ra, w1 = _addr(rgb)
        ya, w2 = _addr(yuv)
        assert w1 == w2
        arr = comps if not isinstance(comps, list) else components(comps)
        _chk(lib().hvc_rgb_to_yuv(self._h, ra, rgb_row_stride, rgb_frame_stride, _rgb_layout(layout), width, height, sampling,
                                  n_frames, ya, yuv_frame_stride, arr, w1), "hvc_rgb_to_yuv")

    def decode_frames_rgb(self, coefs, coef_frame_stride, qtabs, comps, sampling, n_frames, width, height, rgb,
                          layout="interleaved", rgb_row_stride=0, rgb_frame_stride=0):
        """coefficient records -> RGB images: block stage into context scratch, then the colour pass (hvc_decode_frames_rgb)"""
        ca, w1 = _addr(coefs)
        ra, w2 = _addr(rgb)
        assert w1 == w2
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(-1, 64)
        arr = comps if not isinstance(comps, list) else components(comps)
        _chk(lib().hvc_decode_frames_rgb(self._h, ca, coef_frame_stride, q.ctypes.data, q.shape[0], arr, len(arr), sampling,
                                         n_frames, width, height, ra, rgb_row_stride, rgb_frame_stride, _rgb_layout(layout), w1),
             "hvc_decode_frames_rgb")

    def jpeg_decode_rgb(self, data: bytes, layout="interleaved"):
        """one file -> (info, uint8 [h, w, 3] (interleaved) or [3, h, w] (planar))"""
        info = jpeg_read_header(data)
        out = np.zeros(rgb_shape(layout, info.width, info.height), dtype=np.uint8)
        _chk(lib().hvc_jpeg_decode_rgb(self._h, data, len(data), C.byref(info), out.ctypes.data, out.size, 0,
                                       _rgb_layout(layout)), "hvc_jpeg_decode_rgb")
        return info, out

    # -- decoding at 1/2, 1/4, 1/8 size (include/hvc_jpeg.h, "Decoding at reduced size") ----------------------
    def decode_frames_scaled(self, coefs, coef_frame_stride, qtabs, comps, n_frames, scale_denom, pixels, pixel_frame_stride):
        """hvc_decode_frames at 1 / scale_denom: comps place planes of blocks_w * N x blocks_h * N samples, N = 8 / scale_denom"""
        ca, w1 = _addr(coefs)
        pa, w2 = _addr(pixels)
        assert w1 == w2
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(-1, 64)
        arr = comps if not isinstance(comps, list) else components(comps)
        _chk(lib().hvc_decode_frames_scaled(self._h, ca, coef_frame_stride, q.ctypes.data, q.shape[0], arr, len(arr), n_frames,
                                            scale_denom, pa, pixel_frame_stride, w1), "hvc_decode_frames_scaled")

    def jpeg_decode_scaled(self, data: bytes, scale_denom):
        """one file at 1 / scale_denom: (scaled info, its padded pixel record as numpy uint8)"""
        info = jpeg_scaled_info(jpeg_read_header(data), scale_denom)
        pixels = np.zeros(info.pixel_bytes, dtype=np.uint8)
        _chk(lib().hvc_jpeg_decode_scaled(self._h, data, len(data), scale_denom, C.byref(info), pixels.ctypes.data, pixels.size),
             "hvc_jpeg_decode_scaled")
        return info, pixels

    def jpeg_decode_scaled_rgb(self, data: bytes, scale_denom, layout="interleaved"):
        """one file at 1 / scale_denom -> (scaled info, uint8 [h, w, 3] (interleaved) or [3, h, w] (planar))"""
        info = jpeg_scaled_info(jpeg_read_header(data), scale_denom)
        out = np.zeros(rgb_shape(layout, info.width, info.height), dtype=np.uint8)
        _chk(lib().hvc_jpeg_decode_scaled_rgb(self._h, data, len(data), scale_denom, C.byref(info), out.ctypes.data, out.size, 0,
                                              _rgb_layout(layout)), "hvc_jpeg_decode_scaled_rgb")
        return info, out

    def jpeg_decode_batch_scaled(self, jpegs, scale_denom, pixels, pixel_frame_stride, threads=8, frames_per_chunk=0,
                                 gpu_entropy=False):
        """a batch of files of one geometry -> scaled pixel records (numpy: host, torch CUDA tensor: device).  BatchStats."""
        n = len(jpegs)
        ptrs = (C.c_void_p * max(n, 1))(*[C.cast(C.c_char_p(j), C.c_void_p) for j in jpegs])
        sizes = (C.c_size_t * max(n, 1))(*[len(j) for j in jpegs])
        pa, where = _addr(pixels)
        st = BatchStats()
        _chk(lib().hvc_jpeg_decode_batch_scaled(self._h, ptrs, sizes, n, threads, frames_per_chunk, 1 if gpu_entropy else 0,
                                                scale_denom, pa, pixel_frame_stride, where, C.byref(st)),
             "hvc_jpeg_decode_batch_scaled")
        return st

    def jpeg_decode_batch_rgb(self, jpegs, rgb, layout="interleaved", threads=8, frames_per_chunk=0, gpu_entropy=False,
                              rgb_row_stride=0, rgb_frame_stride=0):
        """a batch of files of one geometry -> RGB images in rgb (numpy: host, torch CUDA tensor: device), e.g.
        [n, h, w, 3] / [n, 3, h, w] uint8; gpu_entropy: the Huffman reader on the GPU as well.  Returns BatchStats."""
        n = len(jpegs)
        ptrs = (C.c_void_p * max(n, 1))(*[C.cast(C.c_char_p(j), C.c_void_p) for j in jpegs])
        sizes = (C.c_size_t * max(n, 1))(*[len(j) for j in jpegs])
        ra, where = _addr(rgb)
        st = BatchStats()
        _chk(lib().hvc_jpeg_decode_batch_rgb(self._h, ptrs, sizes, n, threads, frames_per_chunk, 1 if gpu_entropy else 0, ra,
                                             rgb_row_stride, rgb_frame_stride, _rgb_layout(layout), where, C.byref(st)),
             "hvc_jpeg_decode_batch_rgb")
        return st

    def jpeg_encode_rgb(self, rgb, chroma=420, quality=75, layout="interleaved", width=None, height=None):
        """an RGB image ([h, w, 3] or, planar, [3, h, w]; uint8) -> jpeg bytes: hvc_jpeg_encode of the converted planes"""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if width is None:
            height, width = (rgb.shape[1], rgb.shape[2]) if _rgb_layout(layout) == 1 else (rgb.shape[0], rgb.shape[1])
        cap = 4 * width * height + 65536 + self._restart_slack(width, height)
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t()
        _chk(lib().hvc_jpeg_encode_rgb(self._h, rgb.ctypes.data, 0, _rgb_layout(layout), width, height, chroma, quality,
                                       out.ctypes.data, cap, C.byref(n)), "hvc_jpeg_encode_rgb")
        return out[:n.value].tobytes()

    def jpeg_entropy_decode_gpu(self, jpegs, device=False):
        """Huffman decoding of a batch of files on the GPU: (info, coefficient records [n][coef_count], used_gpu)"""
        n = len(jpegs)
        info = jpeg_read_header(jpegs[0])
        ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(j), C.c_void_p) for j in jpegs])
        sizes = (C.c_size_t * n)(*[len(j) for j in jpegs])
        used = C.c_int(-1)
        if device:
            import torch
            # canary elements behind the last record: the reader's write passes must never store past the records,
            # settled stream or not (this wrapper is the harness of the tests and of tools/stress_hdec.py)
            guard = 8192
            buf = torch.full((n * info.coef_count + guard,), 0x5A5A, dtype=torch.int16, device="cuda")
            out = buf[:n * info.coef_count].view(n, info.coef_count)
            torch.cuda.synchronize()
            _chk(lib().hvc_jpeg_entropy_decode_gpu(self._h, ptrs, sizes, n, out.data_ptr(), info.coef_count, 1,
                                                   C.byref(info), C.byref(used)), "hvc_jpeg_entropy_decode_gpu")
            torch.cuda.synchronize()
            if not bool((buf[n * info.coef_count:] == 0x5A5A).all()):
                raise RuntimeError("hvc_jpeg_entropy_decode_gpu wrote past the coefficient records")
            return info, out.cpu().numpy(), used.value
        out = np.empty((n, info.coef_count), dtype=np.int16)
        _chk(lib().hvc_jpeg_entropy_decode_gpu(self._h, ptrs, sizes, n, out.ctypes.data, info.coef_count, 0, C.byref(info),
                                               C.byref(used)), "hvc_jpeg_entropy_decode_gpu")
        return info, out, used.value

    MIXED_READERS = {"host": 0, "gpu": 1}

    def set_mixed_reader(self, which="gpu"):
        """hvc_set_mixed_reader: who reads the files of the mixed batch calls, "host" (the default) or "gpu" -- the mixed GPU
        Huffman reader; which one ran never changes a result"""
        self._set("hvc_set_mixed_reader", self.MIXED_READERS, which)

    def get_mixed_reader(self):
        return {0: "host", 1: "gpu"}[self._get("hvc_get_mixed_reader", -1)]

    def last_mixed_reader_files(self):
        """(gpu_files, host_files) of the last mixed batch call: the files that reached a reader, by the reader that read them"""
        g, h = C.c_uint64(0), C.c_uint64(0)
        _chk(lib().hvc_last_mixed_reader_files(self._h, C.byref(g), C.byref(h)), "hvc_last_mixed_reader_files")
        return g.value, h.value

    def jpeg_entropy_decode_gpu_mixed(self, files, device=False, layout=None, coefs=None):
        """Huffman decoding of files of any geometry on the GPU (hvc_jpeg_entropy_decode_gpu_mixed).  Returns one
        (status, info, record, used_gpu) per file: status = the file's own hvc_status, record = its coefficient record
        (numpy int16 [coef_count]; None unless status is 0), used_gpu = 1 where the GPU reader produced it.
        layout / coefs: a MixedLayout made before and an int16 buffer (numpy, or a torch cuda tensor: then `device` is what
        the buffer says) of at least mixed_coef_offsets(layout)[1] elements to decode into (default: made here)."""
        lay = layout if layout is not None else MixedLayout(files, 8)
        n = len(lay)
        offs, total = mixed_coef_offsets(lay)
        status = (C.c_int * n)(*lay.status)
        used = (C.c_int * n)()
        if coefs is None:
            if device:
                import torch
                coefs = torch.zeros(max(total, 8), dtype=torch.int16, device="cuda")
            else:
                coefs = np.zeros(max(total, 8), dtype=np.int16)
        addr, where = _addr(coefs)
        _chk(lib().hvc_jpeg_entropy_decode_gpu_mixed(self._h, lay.ptrs, lay.sizes, n, lay.infos, status, addr, offs, total, where,
                                                     used), "hvc_jpeg_entropy_decode_gpu_mixed")
        host = coefs.cpu().numpy() if hasattr(coefs, "cpu") else coefs
        out = []
        for f in range(n):
            info = lay.infos[f] if lay.status[f] == 0 else None
            rec = host[offs[f]:offs[f] + info.coef_count].copy() if info is not None and status[f] == 0 else None
            out.append((status[f], info, rec, used[f]))
        return out

    def _restart_slack(self, width, height):
        """what the context's restart interval adds to a file of this size at most.  Not restart_slack(info, ...): the callers
        size their buffers before any JpegInfo of the frame exists, so the 8 x 8 blocks of the luma plane stand in for the MCUs
        (never fewer)."""
        return _interval_slack(-(-width // 8) * -(-height // 8), self.restart_interval)

    def _huffman_coder(self, name, head, n, cap, tail, where, out=None):
        """the tail of the GPU Huffman coder wrappers: name(*head, out, cap, offsets, *tail, where) with an output of cap bytes
        (out: the caller's) and n + 1 offsets in the memory space `where` -- on the device after torch.cuda.synchronize(), what
        was written read back -- cut into the n per-frame segments as bytes"""
        fn = getattr(lib(), name)
        if where == HVC_MEM_DEVICE:
            import torch
            if out is None:
                out = torch.empty(max(cap, 1), dtype=torch.uint8, device="cuda")
            offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            _chk(fn(*head, out.data_ptr(), cap, offs.data_ptr(), *tail, where), name)
            o = offs.cpu().numpy()
            data = out[:int(o[-1])].cpu().numpy()
        else:
            if out is None:
                out = np.empty(max(cap, 1), dtype=np.uint8)
            o = np.zeros(n + 1, dtype=np.uint64)
            _chk(fn(*head, out.ctypes.data, cap, o.ctypes.data, *tail, where), name)
            data = out
        return [data[int(o[f]):int(o[f + 1])].tobytes() for f in range(n)]

    def huffman_encode_frames(self, info, coefs, coef_frame_stride, n_frames, out_cap=None, restart_interval=0):
        """Encoder back end on the GPU: (list of per-frame entropy-coded segments as bytes).  coefs: host
        int16 array or device tensor holding n_frames records.  restart_interval: an RSTn marker every so many MCUs
        (hvc_huffman_encode_frames_restart with the default tables)"""
        if restart_interval:
            return self._huffman_encode_frames_restart(info, coefs, coef_frame_stride, n_frames, out_cap, restart_interval, False)[0]
        ca, where = _addr(coefs)
        cap = out_cap or (n_frames * (info.coef_count // 64) * 243 + 4096)
        return self._huffman_coder("hvc_huffman_encode_frames", (self._h, C.byref(info), ca, coef_frame_stride, n_frames), n_frames,
                                   cap, (), where)

    def _huffman_encode_frames_restart(self, info, coefs, coef_frame_stride, n_frames, out_cap, restart_interval, optimised):
        """hvc_huffman_encode_frames_restart -> (segments, per-frame specs or None)"""
        ca, where = _addr(coefs)
        cap = out_cap or (n_frames * ((info.coef_count // 64) * 243 + restart_slack(info, restart_interval)) + 4096)
        specs = (HuffSpec * max(4 * n_frames, 1))() if optimised else None
        segs = self._huffman_coder("hvc_huffman_encode_frames_restart",
                                   (self._h, C.byref(info), ca, coef_frame_stride, n_frames, int(restart_interval),
                                    HVC_HUFF["optimised" if optimised else "default"]), n_frames, cap, (specs,), where)
        return segs, _spec_pairs(specs, n_frames)

    def huffman_encode_frames_optimised(self, info, coefs, coef_frame_stride, n_frames, out_cap=None, restart_interval=0):
        """hvc_huffman_encode_frames with each frame's own optimal tables, counted and built on the GPU: (list of per-frame
        segments as bytes, list of per-frame [(bits, vals)] x 4: DC0, DC1, AC0, AC1).  restart_interval: an RSTn marker
        every so many MCUs, the tables those of the scan so cut (hvc_huffman_encode_frames_restart)"""
        if restart_interval:
            return self._huffman_encode_frames_restart(info, coefs, coef_frame_stride, n_frames, out_cap, restart_interval, True)
        ca, where = _addr(coefs)
        cap = out_cap or (n_frames * (info.coef_count // 64) * 243 + 4096)
        specs = (HuffSpec * max(4 * n_frames, 1))()
        segs = self._huffman_coder("hvc_huffman_encode_frames_optimised", (self._h, C.byref(info), ca, coef_frame_stride, n_frames),
                                   n_frames, cap, (specs,), where)
        return segs, _spec_pairs(specs, n_frames)

    def jpeg_encode_batch(self, frames, width, height, chroma=420, quality=75, threads=8, frames_per_chunk=16,
                          gpu_entropy=False):
        """Encoder.encode_4xx over a batch of raw planar frames (bytes / uint8 arrays in Frame.input layout).
        Returns (list of jpeg byte strings, BatchStats).  gpu_entropy: Huffman coding on the GPU as well."""
        n = len(frames)
        arrs = _flat_bytes(frames)
        cw = width if chroma == 444 else width // 2
        ch = height // 2 if chroma == 420 else height
        need = width * height + 2 * cw * ch
        for a in arrs:
            if a.size < need:
                raise ValueError("frame shorter than %d bytes" % need)
        cap = 4 * width * height + 65536 + self._restart_slack(width, height)
        outs = [np.empty(cap, dtype=np.uint8) for _ in range(n)]
        fp = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        op = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in outs])
        caps = (C.c_size_t * max(n, 1))(*([cap] * n))
        sizes = (C.c_size_t * max(n, 1))()
        st = BatchStats()
        fn = lib().hvc_jpeg_encode_batch_gpu if gpu_entropy else lib().hvc_jpeg_encode_batch
        _chk(fn(self._h, fp, n, width, height, chroma, quality, threads, frames_per_chunk, op, caps, sizes, C.byref(st)),
             "hvc_jpeg_encode_batch_gpu" if gpu_entropy else "hvc_jpeg_encode_batch")
        return [outs[f][:sizes[f]].tobytes() for f in range(n)], st

    def jpeg_encode_batch_mixed_gpu(self, frames, specs=None, threads=8, chunk_bytes=0, layout=None, caps=None, outs=None):
        """hvc_jpeg_encode_batch_mixed_gpu: jpeg_encode_batch_mixed with the Huffman coder on the GPU too (the mixed coder,
        csrc/hvc_huff_mixed.hip): the same arguments, the same result tuples.  last_mixed_coder_files() says who coded what."""
        return self.jpeg_encode_batch_mixed(frames, specs, threads, chunk_bytes, layout, caps, outs, coder="gpu")

    def last_mixed_coder_files(self):
        """(gpu_files, host_files) of the last jpeg_encode_batch_mixed_gpu call: the files each coder wrote"""
        g, h = C.c_uint64(0), C.c_uint64(0)
        _chk(lib().hvc_last_mixed_coder_files(self._h, C.byref(g), C.byref(h)), "hvc_last_mixed_coder_files")
        return g.value, h.value

    def huffman_encode_frames_mixed(self, infos, coefs, coef_offsets, optimised=False, out_cap=None, out=None):
        """hvc_huffman_encode_frames_mixed: the mixed GPU Huffman coder alone.  Frame f = infos[f] (JpegInfo), its coefficient
        record at coefs[coef_offsets[f]:] (int16 elements; numpy = host, torch cuda tensor = device).  Returns (segments, status,
        specs): per frame its entropy-coded segment as bytes (empty for a refused or flagged frame), its own hvc_status, and --
        optimised -- its [(bits, vals)] x 4 (None where the frame is not good); specs is None with the default tables.
        out_cap: the capacity to offer (default: enough); out: the uint8 output array / tensor to write into (default: made
        here)."""
        n = len(infos)
        m = max(n, 1)
        arr = _infos_array(infos)
        ca, where = _addr(coefs) if coefs is not None else (None, HVC_MEM_HOST)
        cap = out_cap if out_cap is not None else sum((arr[f].coef_count // 64) * 243 for f in range(n)) + 4096
        status = (C.c_int * m)(*([77] * m))
        specs = (HuffSpec * (4 * m))() if optimised else None
        segs = self._huffman_coder("hvc_huffman_encode_frames_mixed",
                                   (self._h, arr, ca, _size_array(coef_offsets, n), n, HVC_HUFF["optimised" if optimised else "default"]),
                                   n, cap, (status, specs), where, out)
        st = [status[f] for f in range(n)]
        return segs, st, _spec_pairs(specs, n, st)

    def jpeg_encode_batch_mixed(self, frames, specs=None, threads=8, chunk_bytes=0, layout=None, caps=None, outs=None, coder="host"):
        """hvc_jpeg_encode_batch_mixed (coder="gpu": hvc_jpeg_encode_batch_mixed_gpu, the Huffman coder on the GPU too): raw planar frames (bytes / uint8 arrays, tight Y, U, V) of any sizes, samplings and
        qualities -> files, in one call.  specs: (width, height, chroma, quality) per frame, or layout: an EncoderMixedLayout
        made before.  Returns one (status, jpeg bytes or None, size) per frame: status = the frame's own hvc_status (0 = a file),
        size = sizes[f] as the call left it (the size needed where caps[f] was too small).  caps / outs (optional): the
        capacity and the uint8 output array of every frame (default: made here, large enough).  The call's hvc_batch_stats:
        self.last_batch_stats."""
        lay = layout if layout is not None else EncoderMixedLayout(specs)
        arrs = _flat_bytes(frames)
        assert len(arrs) == len(lay)
        for f, a in enumerate(arrs):
            if lay.status[f] == 0:
                k = lay.infos[f].comp
                need = sum(k[i].actual_width * k[i].actual_height for i in range(3))
                if a.size < need:
                    raise ValueError("frame %d shorter than %d bytes" % (f, need))
        return self._encode_batch_mixed("hvc_jpeg_encode_batch_mixed", coder, lay, arrs, (), threads, chunk_bytes, caps, outs)

    def _encode_batch_mixed(self, name, coder, lay, arrs, front, threads, chunk_bytes, caps, outs):
        """the tail of the two mixed encode batch calls: name (coder "gpu": name_gpu) (ctx, frames, *front, infos, status, n,
        threads, chunk_bytes, jpegs, caps, sizes, stats) over the flat uint8 arrays `arrs`, into outs / caps (None: made here,
        large enough for any file of the frame's size under the context's restart interval; 8 bytes for a frame the layout
        refused), the stats into self.last_batch_stats -> one (status, jpeg bytes or None, size) per frame"""
        name += {"host": "", "gpu": "_gpu"}[coder]
        n = len(lay)
        m = max(n, 1)
        if outs is None:
            ri = self.restart_interval
            outs = [np.empty(8, dtype=np.uint8) if lay.status[f] else
                    np.empty(4 * lay.infos[f].width * lay.infos[f].height + 65536 + restart_slack(lay.infos[f], ri), dtype=np.uint8)
                    for f in range(n)]
        if caps is None:
            caps = [o.size for o in outs]
        fp = (C.c_void_p * m)(*[a.ctypes.data for a in arrs])
        op = (C.c_void_p * m)(*[o.ctypes.data for o in outs])
        cp = (C.c_size_t * m)(*[int(x) for x in caps])
        sizes = (C.c_size_t * m)()
        status = (C.c_int * m)(*lay.status)
        st = BatchStats()
        _chk(getattr(lib(), name)(self._h, fp, *front, lay.infos, status, n, threads, chunk_bytes, op, cp, sizes, C.byref(st)), name)
        self.last_batch_stats = st
        return [(status[f], outs[f][:sizes[f]].tobytes() if status[f] == 0 else None, sizes[f]) for f in range(n)]

    def jpeg_encode_batch_mixed_rgb(self, images, specs=None, threads=8, chunk_bytes=0, layout="interleaved", rgb_row_strides=None,
                                    enc_layout=None, caps=None, outs=None, coder="host"):
        """hvc_jpeg_encode_batch_mixed_rgb (coder="gpu": hvc_jpeg_encode_batch_mixed_rgb_gpu): RGB images (uint8 arrays, [H, W, 3]
        interleaved or [3, H, W] planar, or flat bytes; rows rgb_row_strides[f] bytes apart, None: tight) of any sizes,
        samplings and qualities -> files, in one call.  specs: (width, height, chroma, quality) per image, or enc_layout: an
        EncoderMixedLayout / EncoderMixedRgbLayout made before.  Results, caps and outs as jpeg_encode_batch_mixed; every file
        equals jpeg_encode_rgb's for that image alone."""
        lay = enc_layout if enc_layout is not None else EncoderMixedRgbLayout(specs, layout)
        code = _rgb_layout(layout)
        arrs = _flat_bytes(images)
        assert len(arrs) == len(lay)
        for f, a in enumerate(arrs):
            if lay.status[f] == 0:
                w, h = lay.infos[f].width, lay.infos[f].height
                tight = w if code == 1 else 3 * w
                rows = 3 * h if code == 1 else h
                rs = (rgb_row_strides[f] if rgb_row_strides is not None else 0) or tight
                if rs >= tight and a.size < (rows - 1) * rs + tight:
                    raise ValueError("image %d shorter than %d bytes" % (f, (rows - 1) * rs + tight))
        return self._encode_batch_mixed("hvc_jpeg_encode_batch_mixed_rgb", coder, lay, arrs, (_size_array(rgb_row_strides, len(lay)), code),
                                        threads, chunk_bytes, caps, outs)

    # -- encode -------------------------------------------------------------
    def encode_frames_mixed(self, pixels, pixel_offsets, infos, coefs, coef_offsets):
        """hvc_encode_frames_mixed: frame f = infos[f] (JpegInfo: layout and tables), its padded pixel record at
        pixels[pixel_offsets[f]:] (bytes), its coefficient record written at coefs[coef_offsets[f]:] (int16 elements).
        pixels / coefs: numpy (host) or torch cuda tensors, both in the same memory space."""
        pa, ca, w1 = _same_space(pixels, "pixels", coefs, "coefs")
        n = len(infos)
        _chk(lib().hvc_encode_frames_mixed(self._h, pa, _size_array(pixel_offsets, n), _infos_array(infos), n, ca,
                                           _size_array(coef_offsets, n), w1), "hvc_encode_frames_mixed")

    def fdct_quant(self, plane, qtab, blocks_w, blocks_h, n_planes, coefs, stride=None, plane_stride=0,
                   coef_plane_stride=0):
        pa, w1 = _addr(plane)
        ca, w2 = _addr(coefs)
        assert w1 == w2
        q = np.ascontiguousarray(qtab, dtype=np.uint16)
        _chk(lib().hvc_fdct_quant(self._h, pa, stride or blocks_w * 8, plane_stride, q.ctypes.data, blocks_w,
                                  blocks_h, n_planes, ca, coef_plane_stride, w1))

    def encode_frames(self, pixels, pixel_frame_stride, qtabs, comps, n_frames, coefs, coef_frame_stride):
        pa, w1 = _addr(pixels)
        ca, w2 = _addr(coefs)
        assert w1 == w2
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(-1, 64)
        arr = comps if not isinstance(comps, list) else components(comps)
        _chk(lib().hvc_encode_frames(self._h, pa, pixel_frame_stride, q.ctypes.data, q.shape[0], arr, len(arr),
                                     n_frames, ca, coef_frame_stride, w1))

    def encode_frames_recon(self, pixels, pixel_frame_stride, qtabs, comps, n_frames, coefs, coef_frame_stride, recon=None,
                            error=None):
        """Encoder.encode_block with ~compute_reconstruction_error:true: coefficients + recon / error records"""
        pa, w1 = _addr(pixels)
        ca, w2 = _addr(coefs)
        ra = _addr(recon)[0] if recon is not None else None
        ea = _addr(error)[0] if error is not None else None
        assert w1 == w2
        q = np.ascontiguousarray(qtabs, dtype=np.uint16).reshape(-1, 64)
        arr = comps if not isinstance(comps, list) else components(comps)
        _chk(lib().hvc_encode_frames_recon(self._h, pa, pixel_frame_stride, q.ctypes.data, q.shape[0], arr, len(arr), n_frames,
                                           ca, coef_frame_stride, ra, ea, w1), "hvc_encode_frames_recon")

    def upsample420(self, src, cw, ch, dst, n_planes=1, src_stride=None, dst_stride=None, src_plane_stride=0,
                    dst_plane_stride=0):
        sa, w1 = _addr(src)
        da, w2 = _addr(dst)
        assert w1 == w2
        _chk(lib().hvc_upsample420(self._h, sa, cw, ch, src_stride or cw, da, dst_stride or 2 * cw, n_planes,
                                   src_plane_stride, dst_plane_stride, w1))

    def _plane_op(self, name, src, sw, sh, dst, dw, n_planes, src_stride, dst_stride, src_plane_stride, dst_plane_stride):
        sa, w1 = _addr(src)
        da, w2 = _addr(dst)
        assert w1 == w2
        _chk(getattr(lib(), name)(self._h, sa, sw, sh, src_stride or sw, da, dst_stride or dw, n_planes, src_plane_stride,
                                  dst_plane_stride, w1), name)

    def subsample420(self, src, sw, sh, dst, n_planes=1, src_stride=None, dst_stride=None, src_plane_stride=0, dst_plane_stride=0):
        """Planar_444.subsample_hv2: sw x sh -> (sw // 2) x (sh // 2)"""
        self._plane_op("hvc_subsample420", src, sw, sh, dst, sw // 2, n_planes, src_stride, dst_stride, src_plane_stride, dst_plane_stride)

    def subsample422(self, src, sw, sh, dst, n_planes=1, src_stride=None, dst_stride=None, src_plane_stride=0, dst_plane_stride=0):
        """Planar_444.subsample_h2: sw x sh -> (sw // 2) x sh"""
        self._plane_op("hvc_subsample422", src, sw, sh, dst, sw // 2, n_planes, src_stride, dst_stride, src_plane_stride, dst_plane_stride)

    def upsample422(self, src, cw, h, dst, n_planes=1, src_stride=None, dst_stride=None, src_plane_stride=0, dst_plane_stride=0):
        """Planar_444.supersample_h2: cw x h -> 2cw x h"""
        self._plane_op("hvc_upsample422", src, cw, h, dst, 2 * cw, n_planes, src_stride, dst_stride, src_plane_stride, dst_plane_stride)

    def crop_planes(self, src, sw, sh, x_pos, y_pos, dst, dw, dh, n_planes=1, src_stride=None, dst_stride=None,
                    src_plane_stride=0, dst_plane_stride=0):
        """Yuv.crop of one plane (clamped source coordinates)"""
        sa, w1 = _addr(src)
        da, w2 = _addr(dst)
        assert w1 == w2
        _chk(lib().hvc_crop_planes(self._h, sa, sw, sh, src_stride or sw, x_pos, y_pos, da, dw, dh, dst_stride or dw, n_planes,
                                   src_plane_stride, dst_plane_stride, w1), "hvc_crop_planes")

    def yuv_convert(self, src, src_format, src_size, dst, dst_format, dst_size, offset=(0, 0), n_frames=1):
        """Oconv.main's loop body: n_frames raw frames of src_format / src_size -> dst_format / dst_size"""
        sa, w1 = _addr(src)
        da, w2 = _addr(dst)
        assert w1 == w2
        _chk(lib().hvc_yuv_convert(self._h, sa, src_format, src_size[0], src_size[1], offset[0], offset[1], da, dst_format,
                                   dst_size[0], dst_size[1], n_frames, w1), "hvc_yuv_convert")
