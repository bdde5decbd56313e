/*
 * hvc_jpeg.h -- C ABI of libhvc_jpeg.so: the MI355X (gfx950) JPEG block-transform
 * path that drops in behind hardcamls/video-coding's `jpeg/model` Decoder /
 * Encoder API.
 *
 * The reference has no FFI layer; this header is the
 * boundary a maintainer binds at the seam `jpeg/model/src/decoder.ml:347-360`
 * (decode_block) and `jpeg/model/src/encoder.ml:195-205` (encode_block).  Each
 * entry point cites the reference code it replaces (paths relative to the
 * reference root).  INTEGRATION.md shows the OCaml ctypes binding.
 *
 * Conventions
 *  - plain C, no exceptions cross the boundary (every entry point is a function-try-block: std::bad_alloc comes
 *    back as HVC_E_OUT_OF_MEMORY, std::system_error as HVC_E_SYSTEM); every function returns
 *    HVC_OK (0) or a negative hvc_status; hvc_strerror() gives a static string.
 *    The OCaml wrapper maps a non-zero code to `raise_s [%message "hvc" ...]`,
 *    the model's own error style (decoder.ml:67, 92, 101, 136).
 *  - the caller owns every buffer it passes; the library never retains a
 *    caller pointer after the call returns (after hvc_synchronize for device
 *    pointers).  Device scratch and streams live inside hvc_ctx.
 *  - an hvc_ctx is bound to ONE GPU and is NOT thread-safe: one per host
 *    thread / GPU.  There is no CPU backend: hvc_create fails with
 *    HVC_E_NO_DEVICE when no gfx950 device is usable.
 *  - all results are bit-exact to the OCaml model: for every coefficient record (int16 coefficients, DC absolute;
 *    8- or 16-bit quantiser entries) and for every file the model decodes.  One thing the int16 RECORD cannot
 *    carry: the model's ints are 63-bit (decoder.ml:143 `dc = coefs.(0) + dc_pred` never wraps), so a malformed-
 *    but-decodable stream whose DC differences pile up to an absolute DC beyond +-32767 (17 blocks of +2047 in a
 *    row do it; no encoder writes that) still decodes there, to saturated blocks.  The entry points that RETURN
 *    records (hvc_jpeg_entropy_decode, hvc_jpeg_entropy_decode_gpu) refuse such a stream with HVC_E_RANGE instead
 *    of wrapping; the entry points that decode FILES TO PIXELS (hvc_jpeg_decode, hvc_jpeg_decode_yuv444, the
 *    hvc_jpeg_decode_batch family) carry those blocks' true DCs on a side list through an int64 fix-up and give the
 *    model's pixels (tests/test_host_entropy.py::test_dc_beyond_int16_is_refused_not_wrapped,
 *    tests/test_gpu_jpeg_api.py::test_dc_beyond_int16_decodes_like_the_model).  That includes DC categories of 17 to
 *    62 bits, which the model reads without complaint (decoder.ml:81-96 asks no question of the table) and then carries
 *    through its 63-bit arithmetic, wrap-around included: the int64 fix-up computes modulo 2^63 as OCaml does
 *    (tests/test_gpu_jpeg_api.py::test_dc_categories_up_to_62_bits).  From 63 bits on, mag' (decoder.ml:73-79) shifts by
 *    Sys.int_size or more, which OCaml leaves unspecified: there is no model result to match, HVC_E_BAD_JPEG.
 *    A component that comes out with ZERO width or height -- a sampling factor of zero other than the first component's,
 *    or a frame dimension of zero -- is the model's empty Plane.t: hvc_jpeg_read_header reports it (blocks_w or blocks_h
 *    of 0), the readers walk the MCUs with no block for it, the block stage skips it, and hvc_jpeg_decode succeeds exactly
 *    where Decoder.decode does; what the model then cannot do is make a Frame.t of such planes, and neither can
 *    hvc_jpeg_get_yuv_frame (see there).  A zero factor in the FIRST component raises in decode_seq (Division_by_zero,
 *    decoder.ml:377-382), in ALL components in init (Int.round_up to a multiple of 0): HVC_E_BAD_JPEG.
 *    An entropy-coded segment of at most 32 bits is decoded with
 *    Bitstream_reader.show's own length test (bitstream_reader.ml:31-33: a request for as many bits as the whole
 *    segment has raises), so such a file is refused or decoded exactly where the model refuses or decodes it
 *    (tests/test_host_entropy.py::test_segments_of_a_few_bytes_raise_where_the_model_does,
 *    ::test_tables_and_headers_the_model_raises_on).  The one input left without a counterpart: a scan with no marker
 *    behind it, on which the model's extract_entropy_coded_bits (decoder.ml:261-281) never returns; here the scan ends
 *    with the file.
 *
 * Data layouts
 *  - coefficients: int16, [plane][blocks_h][blocks_w][64], each block in
 *    ZIG-ZAG order exactly as the model's `coefs` array holds them after
 *    Huffman decoding (decoder.ml:118-140) but with the DC predictor already
 *    added (decoder.ml:143 is a sequential dependency and stays on the host).
 *  - quantiser tables: 64 x uint16 in zig-zag order = Markers.Dqt.elements
 *    (markers.ml:153-167), indexed like `qnt_tab.(i)` at decoder.ml:146.
 *  - pixel planes: row-major uint8, `stride` bytes per row = the model's
 *    Plane.t (common/src/plane.ml:4-17); a Base_bigstring's data pointer can be
 *    passed as is.
 */
#ifndef HVC_JPEG_H
#define HVC_JPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HVC_API __attribute__((visibility("default")))

typedef struct hvc_ctx hvc_ctx; /* opaque: device, stream, scratch, fix-up list */

typedef enum hvc_status {
    HVC_OK = 0,
    HVC_E_INVALID_ARG = -1,  /* null pointer, non-positive size, bad enum */
    HVC_E_NO_DEVICE = -2,    /* no usable gfx950 GPU / HIP runtime error at create */
    HVC_E_HIP = -3,          /* a HIP call failed; hvc_last_hip_error() has the code */
    HVC_E_ALIGNMENT = -4,    /* plane pointer/stride not 8-byte aligned, coefs not 16-byte aligned */
    HVC_E_RANGE = -5,        /* quantiser entry 0 on the ENCODER side (the model divides by it), encoder output outside int16, or (record-returning entry points) a
                                decoded absolute DC outside int16 */
    HVC_E_OUT_OF_MEMORY = -6,
    HVC_E_TOO_LARGE = -7,    /* plane geometry beyond the kernel's index range */
    HVC_E_BAD_JPEG = -8,     /* the model would raise: missing frame/scan/table, invalid Huffman code,
                                coefficient index out of range (decoder.ml:92, 101, 136, 228-243, 291) */
    HVC_E_UNSUPPORTED_MARKER = -9, /* "unsupported marker code" (decoder.ml:67) */
    HVC_E_SYSTEM = -10,      /* the system refused a resource the call needs: a host thread of the batch pipelines
                                could not be started (pids limit, RLIMIT_NPROC); the context stays usable */
    HVC_E_INTERNAL = -11,    /* an unexpected C++ exception was stopped at the boundary (never seen; reported, not thrown) */
    HVC_E_BUSY = -12         /* the slot of an asynchronous submission still holds one: hvc_wait(ctx, slot) first */
} hvc_status;

/* where the data pointers of a call live */
typedef enum hvc_mem {
    HVC_MEM_HOST = 0,   /* host memory: staged through device scratch; call blocks until done */
    HVC_MEM_DEVICE = 1  /* device memory of ctx's GPU: enqueued on ctx's stream, returns at once */
} hvc_mem;

HVC_API int hvc_create(hvc_ctx **out, int device);
HVC_API void hvc_destroy(hvc_ctx *ctx);
HVC_API const char *hvc_strerror(int code);
HVC_API int hvc_last_hip_error(const hvc_ctx *ctx);
/* "hvc_jpeg <version> (gfx950) kernels <id>": <id> = the first 12 hex digits of the SHA-256 of the kernel sources the library
 * was built from (csrc/Makefile KERNEL_ID) -- what ties a committed counter pass (profiles/traffic.json) to a build. */
HVC_API const char *hvc_version(void);

/* The host threads of the batch pipelines (hvc_jpeg_decode_batch*, hvc_jpeg_encode_batch*, the download threads of
 * the host-buffer entry points) live in the context: started by the first call that needs them (more when a later
 * call asks for more `threads`), reused by every call after that, joined by hvc_destroy.  A thread the system refuses
 * to start makes the call return HVC_E_SYSTEM; nothing is left running and the context stays usable.
 * hvc_host_threads reports how many the context holds and how many it has ever started (diagnostic).
 * hvc_host_threads_probe (no context, no GPU): starts `threads` pool threads the way a batch call would, runs an empty
 * task on each and joins them -- HVC_OK or HVC_E_SYSTEM; what tests/test_host_threads.py runs under RLIMIT_NPROC. */
HVC_API int hvc_host_threads(const hvc_ctx *ctx, int *alive, uint64_t *ever_started);
HVC_API int hvc_host_threads_probe(int threads);

/* Which CPUs those threads may run on.  No counterpart in the reference (the model is one
 * thread); it matters on a node with eight GPUs, where eight contexts each start `threads` workers: left alone they
 * wander over both sockets, away from the pinned rings they fill and from their GPU's PCIe root.
 *   cpulist  Linux list format, "0-15,32-47"; "auto" = the CPUs local to the context's GPU (the local_cpulist of its
 *            PCI function in sysfs: its NUMA node); NULL or "" = no restriction (the default).
 * CPUs outside the process's own affinity mask are dropped; HVC_E_INVALID_ARG for a malformed list or one that leaves
 * nothing.  The environment variable HVC_HOST_CPUS, if set, is applied by hvc_create in the same way (an unusable
 * value is ignored there).  hvc_get_host_cpus reports the list in force ("" = none) and the number of CPUs in it. */
HVC_API int hvc_set_host_cpus(hvc_ctx *ctx, const char *cpulist);
HVC_API int hvc_get_host_cpus(const hvc_ctx *ctx, char *out, size_t cap, int *n_cpus);

/* Use an existing HIP stream (hipStream_t passed as void*) so that a host runtime can order this
 * library's kernels with its own work; torch.cuda.current_stream().cuda_stream is such a handle.
 * NULL is a stream too -- HIP's default (null) stream, which is what PyTorch's default stream is --
 * NOT "back to the context's own stream": a fresh hvc_ctx runs on its own non-blocking stream, which
 * does not synchronise with the null stream; hvc_reset_stream returns to it. */
HVC_API int hvc_set_stream(hvc_ctx *ctx, void *hip_stream);
HVC_API int hvc_reset_stream(hvc_ctx *ctx);
HVC_API int hvc_synchronize(hvc_ctx *ctx);

/* HIP-event timer on ctx's stream (for benchmarks): begin, enqueue work, end. */
HVC_API int hvc_timer_begin(hvc_ctx *ctx);
HVC_API int hvc_timer_end(hvc_ctx *ctx, float *elapsed_ms);

/* Per-kernel timing: when enabled, every decode/encode call brackets its
 * dominant kernel (K1 / K3 / the fused 4:4:4 kernel -- not the fix-up or seam
 * kernels) with HIP events on ctx's stream (device-memory calls only); hvc_last_kernel_ms waits
 * for that kernel and returns its duration.  bench.py's roofline figure comes
 * from here. */
HVC_API int hvc_set_profiling(hvc_ctx *ctx, int enabled);
HVC_API int hvc_last_kernel_ms(hvc_ctx *ctx, float *elapsed_ms);
/* durations of the last n (<= 64) profiled calls, oldest first; does not
 * serialise the calls themselves (one event pair per call, ring of 64) */
HVC_API int hvc_kernel_ms_history(hvc_ctx *ctx, float *elapsed_ms, int n);

/* ------------------------------------------------------------------------- */
/* Decode side.
 *
 * hvc_dequant_idct_recon: for every 8x8 block of `n_planes` equally sized
 * component planes computes
 *     dequantize + inverse zig-zag   decoder.ml:142-149 (dc_pred = 0, DC absolute)
 *     Dct.Chen.inverse_8x8           dct.ml:11-107
 *     clip, +128, plane store        decoder.ml:213-224
 * i.e. the body of Decoder.decode_block (decoder.ml:347-360) minus the Huffman
 * part.  Block (bx,by) of plane p reads coefs + p*coef_plane_stride +
 * (by*blocks_w+bx)*64 and writes the 8x8 pixels at plane + p*plane_stride +
 * (by*8+j)*stride + bx*8+i.
 * coef_plane_stride is in int16 elements (0 = blocks_w*blocks_h*64);
 * plane_stride in bytes (0 = stride*blocks_h*8). */
HVC_API int hvc_dequant_idct_recon(hvc_ctx *ctx, const int16_t *coefs, size_t coef_plane_stride,
                                   const uint16_t *qtab, int blocks_w, int blocks_h, int n_planes,
                                   uint8_t *plane, size_t stride, size_t plane_stride, int where);

/* A frame batch in one launch: every frame has the same `n_comp` components
 * (Decoder.Component.t, decoder.ml:167-187; geometry of Decoder.init,
 * decoder.ml:304-345). */
typedef struct hvc_component {
    int blocks_w, blocks_h; /* decoded_width/8, decoded_height/8.  0 x n or n x 0: the model's empty plane (a sampling
                             * factor or frame dimension of zero, decoder.ml:304-345); the DECODING entry points skip such a
                             * component as decode_seq does, the encoding ones refuse it (the model's encoder has none) */
    int qtab;               /* index into qtabs[] */
    int reserved;
    size_t coef_offset;     /* int16 elements from the frame's coefficient record */
    size_t plane_offset;    /* bytes from the frame's pixel record */
    size_t stride;          /* bytes per pixel row (>= blocks_w*8, multiple of 8) */
} hvc_component;

/* coefs + f*coef_frame_stride + comp.coef_offset -> pixels + f*pixel_frame_stride
 * + comp.plane_offset, for f < n_frames.  qtabs: [n_qtabs][64] uint16 (host
 * memory always; tiny).  Same arithmetic as hvc_dequant_idct_recon. */
HVC_API int hvc_decode_frames(hvc_ctx *ctx, const int16_t *coefs, size_t coef_frame_stride,
                              const uint16_t *qtabs, int n_qtabs, const hvc_component *comps,
                              int n_comp, int n_frames, uint8_t *pixels,
                              size_t pixel_frame_stride, int where);

/* The step after the path, fused into it: 4:2:0 coefficient records in,
 * tight 4:4:4 frames out.  Per frame:
 *     the block stage of hvc_decode_frames on the three component planes
 *     Decoder.get_yuv_frame / crop        decoder.ml:403-420  (luma width x height, chroma /2)
 *     Planar_444.convert_from_420         tools/src/planar_444.ml:82-103, 122-131 (supersample_hv2)
 * Output record f = frames + f*frame_stride: planes Y, U, V, each width x height bytes, row-major,
 * stride = width, back to back.  The quarter-resolution chroma planes never reach memory.
 * comps: the 4:2:0 geometry of Decoder.init (blocks_w, blocks_h, qtab, coef_offset are used;
 * plane_offset / stride are ignored); n_comp must be 3, width and height even
 * (Yuv.assert_is_420, tools/src/yuv.ml:104-116) and inside the decoded planes. */
HVC_API int hvc_decode_frames_yuv444(hvc_ctx *ctx, const int16_t *coefs, size_t coef_frame_stride,
                                     const uint16_t *qtabs, int n_qtabs, const hvc_component *comps,
                                     int n_comp, int n_frames, int width, int height, uint8_t *frames,
                                     size_t frame_stride, int where);

/* Diagnostic: which implementation the decode entry points use.  0 = default (k_decode_packed, the
 * int16-pair block-per-lane kernel, with the int64 fix-up for blocks outside its proven range), 1 = the
 * unpacked int32 kernel k_decode_fast, 2 = the int64 kernel for every block, 3 = k_decode_q16, the
 * mapping BASELINE.json's north star describes (one block per quarter wavefront, coefficients staged in
 * LDS between the passes; 1.7x slower).  All four produce identical bytes; tests use
 * this to cross-check independent implementations at full batch sizes. */
HVC_API int hvc_set_decode_kernel(hvc_ctx *ctx, int which);

/* Which ARITHMETIC the decode entry points compute.  HVC_ARITH_MODEL (the default) is the OCaml model's decoder, bit for
 * bit.  HVC_ARITH_HARDCAML is the reference's Hardcaml RTL decoder datapath (jpeg/hardcaml/src), bit for bit: the low 12
 * bits of every coefficient (a 12-bit coefficient bus and DC predictor: an absolute DC is taken mod 4096), dequantisation
 * sext12((q & 0xff) * c mod 4096), the 12-bit fixed-point matrix IDCT of dct.ml (Idct_config: ROM round(4096 * M), pass 1
 * rounded to 4 fractional bits, pass 2 rounded and saturated to [-128, 127]), + 128.  Its output differs from the model's
 * by a few levels (the reference's tests allow 2).  The setting is per context and applies to hvc_dequant_idct_recon,
 * hvc_decode_frames (host and device memory), hvc_decode_frames_submit, hvc_jpeg_decode, hvc_jpeg_decode_batch and
 * hvc_jpeg_decode_batch_gpu; hvc_last_wide_blocks reports 0 after a HARDCAML call (no block needs a fix-up).  The fused
 * 4:4:4 entry points (hvc_decode_frames_yuv444, hvc_jpeg_decode_yuv444, hvc_jpeg_decode_batch_yuv444) have no RTL form:
 * under HARDCAML they return HVC_E_INVALID_ARG and leave their output untouched.  The encoder ignores the setting: it has
 * its own, hvc_set_encode_arithmetic below.
 * HVC_ARITH_LIBJPEG is libjpeg's decoder at its defaults (jidctint.c and fancy upsampling), bit for bit: the section
 * "Bit-exact to libjpeg" below states it and says where it applies.
 * hvc_set_arithmetic: HVC_E_INVALID_ARG for any other value.  The value 2 is NOT an arithmetic and stays refused: LIBJPEG is
 * 3 (hvc_set_decode_kernel has a 2, and a test pins hvc_set_arithmetic(ctx, 2) as an error). */
typedef enum { HVC_ARITH_MODEL = 0, HVC_ARITH_HARDCAML = 1, HVC_ARITH_LIBJPEG = 3 } hvc_arith;
HVC_API int hvc_set_arithmetic(hvc_ctx *ctx, int arith);
HVC_API int hvc_get_arithmetic(const hvc_ctx *ctx, int *arith);

/* How far the RTL datapath strays from the model: the arguments of hvc_decode_frames, and instead of pixels one byte per
 * block, max over its 64 pixels of |model - hardcaml| (test_decoder.ml's max_reconstructed_diff).  For frame f, component
 * k, block (bx, by) the byte is at max_diff + f * diff_frame_stride + (blocks of the components before k) + by * blocks_w
 * + bx; diff_frame_stride >= the frame's blocks (n_frames > 1).  max_diff lives where `where` says, as the records do.
 * Independent of hvc_set_arithmetic.  The model's pixels are made in device scratch and never leave the GPU. */
HVC_API int hvc_decode_frames_divergence(hvc_ctx *ctx, const int16_t *coefs, size_t coef_frame_stride,
                                         const uint16_t *qtabs, int n_qtabs, const hvc_component *comps, int n_comp,
                                         int n_frames, uint8_t *max_diff, size_t diff_frame_stride, int where);

/* Which arithmetic the ENCODE entry points compute, independent of hvc_set_arithmetic.  HVC_ARITH_MODEL (the default) is
 * the OCaml model's encoder, bit for bit.  HVC_ARITH_HARDCAML is the finished half of the reference's Hardcaml RTL
 * encoder datapath (jpeg/hardcaml/src/encoder_datapath.ml), bit for bit: p - 128, the 12-bit fixed-point matrix DCT of
 * dct.ml (Dct_config: ROM round(4096 * F), pass 1 rounded to 4 fractional bits, pass 2 rounded and saturated to 12 bits),
 * and quant.ml's reciprocal quantiser, q = RND(R * (4096 / t), 12) (ties away from zero) wrapped to 12 bits.  The
 * coefficient at natural position k is divided by table[Zigzag.forward[k]] and stored at record position
 * Zigzag.forward[k], DC absolute: the DQT table convention of the model's Encoder.quant, so that the files decode as they
 * should (the RTL's own test bench loads its table RAM in raster order, one of the upstream datapath's unfinished parts,
 * with its run-length and Huffman stages, which are not reproduced: the records go to this library's entropy coders).
 * Its coefficients differ from the model's by a few levels.  The setting is per context and applies to hvc_fdct_quant,
 * hvc_encode_frames (host and device memory), hvc_encode_frames_submit, hvc_jpeg_encode, hvc_jpeg_encode_batch,
 * hvc_jpeg_encode_batch_gpu and the encode step of hvc_encode_frames_recon (whose decode step follows hvc_set_arithmetic).
 * Tables are validated as before (1..255, else HVC_E_RANGE).  hvc_set_encode_arithmetic: HVC_E_INVALID_ARG for any other
 * value, the setting unchanged. */
HVC_API int hvc_set_encode_arithmetic(hvc_ctx *ctx, int arith);
HVC_API int hvc_get_encode_arithmetic(const hvc_ctx *ctx, int *arith);

/* How far the RTL encoder's arithmetic strays from the model: the arguments of hvc_encode_frames, and instead of records
 * one byte per block, min(255, max over its 64 coefficients of |q_model - q_hardcaml|).  For frame f, component k, block
 * (bx, by) the byte is at max_diff + f * diff_frame_stride + (blocks of the components before k) + by * blocks_w + bx;
 * diff_frame_stride >= the frame's blocks (n_frames > 1).  max_diff lives where `where` says, as the pixels do.
 * Independent of both settings.  The model's records are made in device scratch and never leave the GPU. */
HVC_API int hvc_encode_frames_divergence(hvc_ctx *ctx, const uint8_t *pixels, size_t pixel_frame_stride,
                                         const uint16_t *qtabs, int n_qtabs, const hvc_component *comps, int n_comp,
                                         int n_frames, uint8_t *max_diff, size_t diff_frame_stride, int where);

/* Number of blocks the last decode call on ctx routed through the wide
 * (64-bit) fix-up kernel (diagnostic; synchronises the stream). */
HVC_API int hvc_last_wide_blocks(hvc_ctx *ctx, uint64_t *count);

/* ------------------------------------------------------------------------- */
/* Encode side (mirror): level shift, Dct.Chen.forward_8x8, quantise, zig-zag
 *     Encoder.level_shifted_input_block  encoder.ml:81-90
 *     Dct.Chen.forward_8x8               dct.ml:109-196
 *     Encoder.quant / quant_and_scale    encoder.ml:98-108
 * Output coefficients in zig-zag order, DC absolute (the DC difference of
 * encoder.ml:138-140 stays on the host with the RLE/Huffman writer). */
HVC_API int hvc_fdct_quant(hvc_ctx *ctx, const uint8_t *plane, size_t stride, size_t plane_stride,
                           const uint16_t *qtab, int blocks_w, int blocks_h, int n_planes,
                           int16_t *coefs, size_t coef_plane_stride, int where);

HVC_API int hvc_encode_frames(hvc_ctx *ctx, const uint8_t *pixels, size_t pixel_frame_stride,
                              const uint16_t *qtabs, int n_qtabs, const hvc_component *comps,
                              int n_comp, int n_frames, int16_t *coefs, size_t coef_frame_stride,
                              int where);

/* hvc_encode_frames plus the debugging tail of Encoder.encode_block (encoder.ml:195-205) that an encoder created
 * with ~compute_reconstruction_error:true runs on every block -- from the block's quantised coefficients
 *     Encoder.dequant   encoder.ml:110-117   quant.(i) * table.(i) through Zigzag.inverse
 *     Encoder.idct      encoder.ml:94-96     Dct.Chen.inverse_8x8
 *     Encoder.recon     encoder.ml:119-125   recon = max 0 (min 255 (idct + 128)); error = abs (recon - input pixel)
 * recon and error (either may be NULL) are pixel records with the layout of `pixels` (same comps, strides and
 * frame stride; bytes outside the component planes are not touched): Block.Decoded.recon / .error of every
 * block at the block's place.  max 0 (min 255 (x + 128)) is the decoder's clip + level shift (decoder.ml:213-224),
 * so recon is also exactly what Decoder.decode will make of the file. */
HVC_API int hvc_encode_frames_recon(hvc_ctx *ctx, const uint8_t *pixels, size_t pixel_frame_stride,
                                    const uint16_t *qtabs, int n_qtabs, const hvc_component *comps, int n_comp,
                                    int n_frames, int16_t *coefs, size_t coef_frame_stride, uint8_t *recon,
                                    uint8_t *error, int where);

/* ------------------------------------------------------------------------- */
/* 4:2:0 -> 4:4:4 chroma upsample, tools/src/planar_444.ml:82-103
 * (supersample_hv2 over all rows, :122-131): src cw x ch -> dst 2cw x 2ch. */
HVC_API int hvc_upsample420(hvc_ctx *ctx, const uint8_t *src, int cw, int ch, size_t src_stride,
                            uint8_t *dst, size_t dst_stride, int n_planes, size_t src_plane_stride,
                            size_t dst_plane_stride, int where);

/* The rest of `oyuv convert` (tools/src/oconv.ml): the other resampling steps of Planar_444, plane by plane like
 * hvc_upsample420 (n_planes planes, src_plane_stride / dst_plane_stride bytes apart, 0 = tight; host or device memory):
 *   hvc_subsample420   Planar_444.subsample_hv2 over all rows (planar_444.ml:69-80, convert_to_420 :105-116):
 *                      src sw x sh -> dst (sw / 2) x (sh / 2), dst[c, r] = (a + b + c + d + 2) >> 2 of the 2 x 2 samples
 *   hvc_subsample422   Planar_444.subsample_h2 (planar_444.ml:18-23, convert_to_422 :35-44): src sw x sh -> dst (sw / 2) x sh
 *   hvc_upsample422    Planar_444.supersample_h2 (planar_444.ml:25-33, convert_from_422 :55-67): src cw x h -> dst 2cw x h,
 *                      dst[2c] = src[c], dst[2c + 1] = avg2 src[c] src[c + 1], the last column twice
 *   hvc_crop_planes    Yuv.crop (tools/src/yuv.ml:42-62) of one plane: dst[c, r] = src[clamp (c + x_pos), clamp (r + y_pos)]
 *                      -- a crop, an offset, and edge replication where the destination reaches past the source */
HVC_API int hvc_subsample420(hvc_ctx *ctx, const uint8_t *src, int sw, int sh, size_t src_stride, uint8_t *dst,
                             size_t dst_stride, int n_planes, size_t src_plane_stride, size_t dst_plane_stride, int where);
HVC_API int hvc_subsample422(hvc_ctx *ctx, const uint8_t *src, int sw, int sh, size_t src_stride, uint8_t *dst,
                             size_t dst_stride, int n_planes, size_t src_plane_stride, size_t dst_plane_stride, int where);
HVC_API int hvc_upsample422(hvc_ctx *ctx, const uint8_t *src, int cw, int h, size_t src_stride, uint8_t *dst,
                            size_t dst_stride, int n_planes, size_t src_plane_stride, size_t dst_plane_stride, int where);
HVC_API int hvc_crop_planes(hvc_ctx *ctx, const uint8_t *src, int sw, int sh, size_t src_stride, int x_pos, int y_pos,
                            uint8_t *dst, int dw, int dh, size_t dst_stride, int n_planes, size_t src_plane_stride,
                            size_t dst_plane_stride, int where);

/* Yuv_format.t (tools/src/yuv_format.ml): the planar formats by their usual number, the packed 4:2:2 ones by name */
enum { HVC_YUV_420 = 420, HVC_YUV_422 = 422, HVC_YUV_444 = 444, HVC_YUV_YUY2 = 1, HVC_YUV_UYVY = 2, HVC_YUV_YVYU = 3 };
/* bytes of one raw frame: Planar.create / Packed.create (yuv_format.ml:21-53: integer halves; packed = 2 * width * height) */
HVC_API int hvc_yuv_frame_bytes(int format, int width, int height, size_t *bytes);
/* Oconv.main's loop body (oconv.ml:111-133) for n_frames raw frames, back to back in `src` and `dst`:
 *   Oconv.input   the source format to a 4:4:4 frame (Packed_422.convert_to_planar, Planar_444.convert_from_420 / _422)
 *   Yuv.crop      ~x_pos:x_off ~y_pos:y_off into a dst_w x dst_h 4:4:4 frame (clamped source coordinates)
 *   Oconv.output  the destination format (Planar_444.convert_to_420 / _422, Packed_422.convert_from_planar)
 * HVC_E_INVALID_ARG where Yuv.assert_is_420 / _422 raise: an odd width for a subsampled format, an odd height for 4:2:0. */
HVC_API int hvc_yuv_convert(hvc_ctx *ctx, const uint8_t *src, int src_format, int src_w, int src_h, int x_off, int y_off,
                            uint8_t *dst, int dst_format, int dst_w, int dst_h, int n_frames, int where);

/* ------------------------------------------------------------------------- */
/* Host front end / back end around the block stage:
 * the callers and data formats either side of the hot path.  Host C++ only. */

typedef struct hvc_jpeg_component { /* Decoder.Component.t geometry, decoder.ml:167-187, 304-345 */
    int identifier, hscale, vscale;
    int decoded_width, decoded_height; /* padded plane: rounded to the MCU */
    int actual_width, actual_height;   /* cropped size of get_yuv_frame */
    int dc_table, ac_table;            /* Huffman table selectors of the scan */
} hvc_jpeg_component;

typedef struct hvc_jpeg_info {
    int width, height, n_comp;     /* Markers.Sof / Sos; components in scan order */
    int n_qtabs;
    hvc_jpeg_component comp[4];
    hvc_component layout[4];       /* tight frame record: planes / coefficient planes back to back */
    uint16_t qtabs[4][64];         /* tables layout[].qtab refers to (Markers.Dqt.elements order) */
    size_t coef_count;             /* int16 elements of one frame's coefficient record */
    size_t pixel_bytes;            /* bytes of one frame's padded pixel record */
    size_t ecs_offset;             /* byte offset of the entropy-coded segment */
} hvc_jpeg_info;

/* Decoder.Header.decode (decoder.ml:36-70) + the geometry of Decoder.init (:294-345). */
HVC_API int hvc_jpeg_read_header(const uint8_t *jpeg, size_t n, hvc_jpeg_info *info);
/* The Huffman + DC-prediction half of Decoder.decode in decode_seq order (decoder.ml:118-140, 143,
 * 261-281, 362-395) into one frame's coefficient record (host memory, info->coef_count int16). */
HVC_API int hvc_jpeg_entropy_decode(const uint8_t *jpeg, size_t n, const hvc_jpeg_info *info, int16_t *coefs);
/* An EXTENSION, off unless asked for: restart intervals (DRI + RSTn markers, ITU-T T.81 B.2.4.4, E.2.4).  The model parses
 * DRI and never looks at it again; its entropy-coded segment ends at the first RSTn as at any marker (decoder.ml:56-59,
 * 261-281), so it decodes the first interval and reads zeros from there on -- and so does every entry point of this library
 * by default (model parity).  hvc_jpeg_entropy_decode_restart is hvc_jpeg_entropy_decode with the markers honoured: every
 * interval's bytes behind its RSTn, DC predictors back to zero at each (SURVEY.md 8f next-1's named extension);
 * hvc_set_restart_markers(ctx, 1) makes the context's file-level entry points (hvc_jpeg_decode, hvc_jpeg_decode_yuv444, the
 * batch pipelines, hvc_jpeg_entropy_decode_gpu) do the same -- the host reader by walking from interval to interval, the GPU
 * reader by taking every interval as a stream of its own (an RSTn is a synchronisation point known in advance: a byte
 * boundary, the first block of an MCU, predictors at zero); files of one batch whose DRI differs from the first file's, or
 * whose markers are not the ones their DRI promises, are the host reader's.  A file without DRI decodes the same either way.
 * Which reader takes a call never changes its result, only its speed; the GPU reader's limits with the extension on are:
 * intervals-per-file x files of one call <= 65535 (hvc_jpeg_entropy_decode_gpu: *used_gpu = 0 past that), intervals per
 * file <= 4096 in the batch pipeline (the whole batch goes through the host-reader pipeline past that), and one DRI per
 * chunk (a chunk holding a file with another DRI is redone by the host reader; stats->entropy_ms_sum > 0 says some were).
 * A scan of a single interval (MCUs <= DRI) is read as the plain segment by both readers. */
HVC_API int hvc_jpeg_entropy_decode_restart(const uint8_t *jpeg, size_t n, const hvc_jpeg_info *info, int16_t *coefs);
HVC_API int hvc_set_restart_markers(hvc_ctx *ctx, int honour);
/* The same for TWO files on the calling thread, their symbols decoded in turn: a file is one stream and its symbols one
 * dependency chain (shift, table load, shift), two files are two chains the core overlaps -- 1.07x (Zen 5) to 1.3x (Golden
 * Cove) the files per second per thread on the bench's content (what the batch pipelines' workers do).  *status_a / *status_b receive
 * what hvc_jpeg_entropy_decode would have returned for each file; an error in one does not stop the other. */
HVC_API int hvc_jpeg_entropy_decode2(const uint8_t *jpeg_a, size_t n_a, const hvc_jpeg_info *info_a, int16_t *coefs_a,
                                     int *status_a, const uint8_t *jpeg_b, size_t n_b, const hvc_jpeg_info *info_b,
                                     int16_t *coefs_b, int *status_b);
/* Decoder.get_yuv_frame (decoder.ml:403-420): the crops of components 0, 1, 2 back to back (Frame.output order,
 * common/src/frame.ml:66-70) -- where Frame.of_planes (frame.ml:42-61) makes a frame of them: three components at least,
 * chroma planes of one size, and that size the luma plane's halved both ways, halved in width, or equal (C420 / C422 /
 * C444 by integer halves).  HVC_E_BAD_JPEG where of_planes raises (4:1:1, 4:4:0, one or two components, an empty plane
 * beside planes with samples); a fourth component is left out, as in the model.  *out_len: the bytes of the frame. */
HVC_API int hvc_jpeg_get_yuv_frame(const hvc_jpeg_info *info, const uint8_t *pixels, uint8_t *out, size_t cap,
                                   size_t *out_len);
/* Decoder.crop (decoder.ml:403-413) mapped over Decoder.get_decoded_planes (:399-401): EVERY component's crop back to
 * back in scan order, whatever the sampling -- for the files whose planes Frame.of_planes has no name for. */
HVC_API int hvc_jpeg_get_cropped_planes(const hvc_jpeg_info *info, const uint8_t *pixels, uint8_t *out, size_t cap,
                                        size_t *out_len);
/* Decoder.decode_a_frame minus the crop (decoder.ml:422-427): header, host entropy decode, GPU block
 * stage; `pixels` (host, info->pixel_bytes) receives the padded planes = get_decoded_planes. */
HVC_API int hvc_jpeg_decode(hvc_ctx *ctx, const uint8_t *jpeg, size_t n, hvc_jpeg_info *info, uint8_t *pixels,
                            size_t pixel_cap);

/* The same for a 4:2:0 file, straight to a tight 4:4:4 frame (hvc_decode_frames_yuv444):
 * decode_a_frame (decoder.ml:422-427) followed by Planar_444.of_420 (tools/src/planar_444.ml:133-137),
 * i.e. `model.exe decode frame` + `oyuv convert -format 420 ... 444`.  frame: 3 * width * height bytes.
 * HVC_E_INVALID_ARG for any other sampling or an odd frame size (Yuv.assert_is_420). */
HVC_API int hvc_jpeg_decode_yuv444(hvc_ctx *ctx, const uint8_t *jpeg, size_t n, hvc_jpeg_info *info,
                                   uint8_t *frame, size_t frame_cap);

/* BASELINE config 3: a batch of baseline JPEGs of identical geometry and tables.  `threads` host
 * threads run the entropy decode into pinned chunk buffers; each finished chunk goes to the GPU with
 * hipMemcpyAsync on a copy stream while the block-stage kernel of the previous chunk runs on the
 * compute stream and the host decodes the next one.  pixels: n padded pixel records
 * (pixel_frame_stride bytes apart; `where` says host or device memory). */
typedef struct hvc_batch_stats {
    double wall_ms, entropy_ms_sum, h2d_ms_sum, kernel_ms_sum, d2h_ms_sum; /* sums over chunks */
    int chunks, threads, frames_per_chunk;
    uint64_t coef_bytes;
    double host_prep_ms_sum; /* hvc_jpeg_encode_batch: plane padding into the pinned ring, summed over threads */
} hvc_batch_stats;
HVC_API int hvc_jpeg_decode_batch(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_frames,
                                  int threads, int frames_per_chunk, uint8_t *pixels, size_t pixel_frame_stride,
                                  int where, hvc_batch_stats *stats);
/* The same pipeline ending in the fused kernel: 4:2:0 files in, tight 4:4:4 frames out (3 * width *
 * height bytes each, frame_stride apart) -- hvc_jpeg_decode_yuv444 for a batch. */
HVC_API int hvc_jpeg_decode_batch_yuv444(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes,
                                         int n_frames, int threads, int frames_per_chunk, uint8_t *frames,
                                         size_t frame_stride, int where, hvc_batch_stats *stats);

/* Quant_tables.scale Quant_tables.luma/chroma quality (quant_tables.ml:139-147). */
HVC_API int hvc_quant_table(int chroma_table, int quality, uint16_t *out64);

/* The cram tests' verification harness (`oyuv compare`, tools/src/ocompare.ml:6-47):
 * max_difference, total_difference and square_error of two planes of n bytes (host memory).
 * mean_difference / mean_square_error / psnr (:30-59) are one float operation on top
 * (video-coding_amd/yuv.py).  Any of the three outputs may be NULL. */
HVC_API int hvc_compare_planes(const uint8_t *a, const uint8_t *b, size_t n, int *max_difference,
                               uint64_t *total_difference, uint64_t *square_error);
/* Encoder.Parameters.c420/c422/c444 + Encoder.create geometry (encoder.ml:287-349, 437-472): chroma is
 * 420, 422 or 444.  Fills the padded plane layout (zero padding, plane.ml:11-17) and the tables. */
HVC_API int hvc_jpeg_encoder_layout(int width, int height, int chroma, int quality, hvc_jpeg_info *info);
/* hvc_jpeg_decode_batch (or _yuv444 when yuv444 != 0) with the Huffman reader on the GPU as well
 * (hvc_jpeg_entropy_decode_gpu below): host threads only parse headers and unstuff the entropy-coded
 * segments into a pinned ring, ~1 MB per 1080p frame crosses PCIe instead of 6 MB of coefficients, and
 * the coefficient records are produced where the block stage reads them.  Every file is read with ITS OWN
 * Huffman tables (decoder.ml:238-259: the DHT segments of the file): a chunk whose files all carry the first
 * file's tables runs with them in LDS, any other chunk with per-frame tables in device memory -- a batch of files
 * with per-file optimised tables stays on the GPU.  Chunks holding a file that needs the host decoder (see
 * below) are redone by the host-decoder pipeline once the others are through: same output, same errors
 * (stats->entropy_ms_sum is the host decoding time spent on them, 0 when the GPU reader did everything).
 * frames_per_chunk < 1 = a quarter of the batch, between 64 and 256 (what measured best). */
HVC_API int hvc_jpeg_decode_batch_gpu(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_frames,
                                      int threads, int frames_per_chunk, uint8_t *pixels,
                                      size_t pixel_frame_stride, int where, int yuv444, hvc_batch_stats *stats);

/* Huffman DEcoding on the GPU (csrc/hvc_hdec.hip): the entropy-coded segments of n_frames files (one
 * geometry; Huffman tables per file) -> coefficient records exactly as
 * hvc_jpeg_entropy_decode writes them.  The segment is cut into 1024-bit subsequences, one lane each;
 * lanes start from guessed states, adopt their predecessor's exit state round after round until nothing
 * changes (Huffman streams re-synchronise), then decode once more writing coefficients; a prefix sum
 * resolves the DC predictor (decoder.ml:143).  Whatever the model raises on, a DC outside int16, tables
 * that are no prefix code, or a stream that ends early makes the call fall back to the host decoder, so the
 * result (and every error code) is the host decoder's.  *used_gpu (optional) tells which one ran.
 * info receives the header of jpegs[0].  The call returns when the records are complete. */
HVC_API int hvc_jpeg_entropy_decode_gpu(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_frames,
                                        int16_t *coefs, size_t coef_frame_stride, int where, hvc_jpeg_info *info,
                                        int *used_gpu);

/* The encoder's back end ON THE GPU (csrc/hvc_huff.hip): Encoder.rle + write_bits + Bitstream_writer
 * with byte stuffing and flush_with_1s (encoder.ml:127-193, 507-510; bitstream_writer.ml) for n_frames
 * coefficient records, as data-parallel passes -- every block's bit string depends only on its own
 * coefficients and on the DC of the block before it in scan order.  Frame f's entropy-coded segment
 * (what stands between the SOS header and EOI) is out[offsets[f] .. offsets[f+1]); offsets has
 * n_frames + 1 entries.  coefs, out and offsets live where `where` says; the call returns when the
 * result is complete (it has to read the status back).  HVC_E_RANGE: a value without a code in the
 * default tables (as hvc_jpeg_entropy_encode); HVC_E_INVALID_ARG: out_cap too small.
 * hvc_jpeg_header gives the bytes in front of the segment (SOI .. SOS); 0xFF 0xD9 (EOI) closes the file. */
HVC_API int hvc_huffman_encode_frames(hvc_ctx *ctx, const hvc_jpeg_info *info, const int16_t *coefs,
                                      size_t coef_frame_stride, int n_frames, uint8_t *out, size_t out_cap,
                                      uint64_t *offsets, int where);
HVC_API int hvc_jpeg_header(const hvc_jpeg_info *info, uint8_t *out, size_t cap, size_t *len);
/* Diagnostic: the code tables the encoder's back ends emit from -- Tables.Encoder.dc_table / ac_table of the default
 * specifications (tables.ml:27-45 canonical assignment, :504-545; Tables.Default = ITU-T T.81 Annex K.3), which the
 * reference's own test prints in full (jpeg/model/test/test_tables.ml:4-395 -> tests/golden/g8_code_tables.json).
 * table_set: 0 luma, 1 chroma.  codes[i] = (code << 5) | length, 0 = no code: i < 16 the DC category i, i = 16 +
 * ((run << 4) | size) the AC symbol.  where = HVC_MEM_HOST: the host coder's tables (ctx may be NULL); HVC_MEM_DEVICE:
 * the GPU coder's tables as they sit in ctx's device memory (uploaded if no call has needed them yet, then read back). */
HVC_API int hvc_huffman_code_tables(hvc_ctx *ctx, int table_set, int where, uint32_t *codes272);

/* HVC_OK when Encoder.encode_seq can walk this geometry; HVC_E_INVALID_ARG where the model raises
 * "[Plane.get] out of bounds" (encoder.ml:476-505 with plane.ml:43-50): the MCU grid of the luma
 * component reaches past a chroma plane for 4:2:0 / 4:2:2 frames of width (or height) 16k + 1.  The
 * encode entry points below return the same error for such frames. */
HVC_API int hvc_jpeg_encoder_check(const hvc_jpeg_info *info);
/* Encoder.write_headers + rle + write_bits + EOI over a coefficient record (encoder.ml:127-193,
 * 371-418, 476-510): byte-identical to Model.Encoder's output. */
HVC_API int hvc_jpeg_entropy_encode(const hvc_jpeg_info *info, const int16_t *coefs, uint8_t *out, size_t cap,
                                    size_t *out_len);
/* Encoder.encode_420/422/444 ~frame ~quality (encoder.ml:512-541): y/u/v are the tight planes of the
 * frame (Frame.create sizes); padding on the host, forward block stage AND Huffman coder on the GPU
 * (only the entropy-coded segment is downloaded), header + segment + EOI assembled into out. */
HVC_API int hvc_jpeg_encode(hvc_ctx *ctx, const uint8_t *y, const uint8_t *u, const uint8_t *v, int width,
                            int height, int chroma, int quality, uint8_t *out, size_t cap, size_t *out_len);

/* ------------------------------------------------------------------------- */
/* Per-file OPTIMISED Huffman tables (an extension: the model's encoder writes the default Annex K tables only).
 * An hvc_huff_spec is the body of one DHT: bits[l - 1] codes of length l, then n_vals symbols (HUFFVAL).  Arrays of four
 * are ordered DC0, DC1, AC0, AC1 (table set 0 = luma, 1 = chroma, as the default files use them).  The header keeps the
 * default files' layout (SOI, APP0, DQT x 2, SOF0, DHT DC0, DC1, AC0, AC1, SOS); only the DHT bodies change.
 *
 * The tables of a file are those of ITU-T T.81 Annex K.2 over its symbol counts (DC categories; (run << 4) | size, ZRL
 * and EOB for AC, as the scan codes them): the reserved 257th symbol with count 1; c1 the LARGEST index among the
 * smallest non-zero counts, c2 likewise with c2 != c1; lengths limited to 16 by figure K.3; the reserved code removed
 * from the longest length; HUFFVAL ordered by the unadjusted code size, then by symbol.  Codes are assigned canonically
 * (tables.ml:27-45).  A DC category above 11 or an AC size above 10 is HVC_E_RANGE, as with the default tables.
 *
 * hvc_set_huffman_tables(ctx, HVC_HUFF_OPTIMISED) makes hvc_jpeg_encode, hvc_jpeg_encode_batch and
 * hvc_jpeg_encode_batch_gpu write such files; it combines with hvc_set_encode_arithmetic.  HVC_HUFF_DEFAULT (the
 * default) leaves every byte as before.  Any other value: HVC_E_INVALID_ARG, the setting unchanged. */
typedef enum { HVC_HUFF_DEFAULT = 0, HVC_HUFF_OPTIMISED = 1 } hvc_huff_tables;
typedef struct hvc_huff_spec {
    uint8_t bits[16];
    uint8_t vals[256];
    uint16_t n_vals;
    uint16_t pad;
} hvc_huff_spec;
HVC_API int hvc_set_huffman_tables(hvc_ctx *ctx, int which);
HVC_API int hvc_get_huffman_tables(const hvc_ctx *ctx, int *which);
/* Annex K.2 over 256 symbol counts (host, no context).  HVC_E_INVALID_ARG when every count is 0, HVC_E_RANGE when they
 * sum past 2^62. */
HVC_API int hvc_huffman_spec_from_counts(const uint64_t counts[256], hvc_huff_spec *out);
/* The four optimal specs of one frame's coefficient record (the geometry of hvc_jpeg_entropy_encode). */
HVC_API int hvc_huffman_optimal_tables(const hvc_jpeg_info *info, const int16_t *coefs, hvc_huff_spec out[4]);
/* hvc_jpeg_header with the given DHT bodies. */
HVC_API int hvc_jpeg_header_tables(const hvc_jpeg_info *info, const hvc_huff_spec specs[4], uint8_t *out, size_t cap,
                                   size_t *len);
/* hvc_jpeg_entropy_encode with the given tables: the whole file.  HVC_E_RANGE for a symbol without a code in specs;
 * HVC_E_INVALID_ARG for a malformed spec (bits that do not sum to n_vals, a Kraft sum above 1, a repeated symbol, a DC
 * symbol above 11). */
HVC_API int hvc_jpeg_entropy_encode_tables(const hvc_jpeg_info *info, const hvc_huff_spec specs[4], const int16_t *coefs,
                                           uint8_t *out, size_t cap, size_t *out_len);
/* hvc_huffman_encode_frames with each frame's own optimal tables, counted and built on the GPU (k_huff_hist,
 * k_huff_build, csrc/hvc_huff.hip).  specs is host memory of n_frames x 4 entries and receives each frame's tables; the
 * segments equal hvc_jpeg_entropy_encode_tables' with them.  An info whose components all select one table set leaves the
 * other without a symbol to fit a table to: HVC_E_INVALID_ARG, as from hvc_huffman_optimal_tables. */
HVC_API int hvc_huffman_encode_frames_optimised(hvc_ctx *ctx, const hvc_jpeg_info *info, const int16_t *coefs,
                                                size_t coef_frame_stride, int n_frames, uint8_t *out, size_t out_cap,
                                                uint64_t *offsets, hvc_huff_spec *specs, int where);

/* ------------------------------------------------------------------------- */
/* Files WITH RESTART INTERVALS (an extension: the model's encoder writes none; ITU-T T.81 B.2.4.4, E.1.4).  With an
 * interval of Ri MCUs (1 .. 65535) the header carries one DRI segment (FF DD 00 04 Ri) directly in front of SOS, nothing
 * else of its layout changes; in front of every MCU whose index m > 0 is a multiple of Ri the pending bits are padded with
 * ones to a byte (stuffed like any other byte if it is 0xFF), the two bytes FF D0+((m / Ri - 1) mod 8) follow unstuffed and
 * every component's DC predictor starts again at 0.  No marker stands behind the last interval.  Ri >= the number of MCUs:
 * the DRI segment is written, no marker is, and the entropy-coded segment is the plain one.  With optimised tables the
 * symbol counts are those of the scan as coded with the interval (the DC categories change where a predictor was reset).
 *
 * hvc_set_restart_interval(ctx, Ri) makes hvc_jpeg_encode, hvc_jpeg_encode_batch and hvc_jpeg_encode_batch_gpu write such
 * files; it combines with hvc_set_huffman_tables and hvc_set_encode_arithmetic and is independent of the READER's
 * hvc_set_restart_markers (which is what reads these files back in full).  0 (the default) leaves every byte as before.
 * A value outside 0 .. 65535: HVC_E_INVALID_ARG, the setting unchanged. */
HVC_API int hvc_set_restart_interval(hvc_ctx *ctx, int mcus);
HVC_API int hvc_get_restart_interval(const hvc_ctx *ctx, int *mcus);
/* hvc_jpeg_header / hvc_jpeg_header_tables with the interval's DRI segment; specs == NULL: the default tables. */
HVC_API int hvc_jpeg_header_restart(const hvc_jpeg_info *info, const hvc_huff_spec *specs, int restart_interval,
                                    uint8_t *out, size_t cap, size_t *len);
/* hvc_jpeg_entropy_encode / hvc_jpeg_entropy_encode_tables with the interval: the whole file (host, no context).
 * restart_interval = 0 gives their bytes. */
HVC_API int hvc_jpeg_entropy_encode_restart(const hvc_jpeg_info *info, const hvc_huff_spec *specs, int restart_interval,
                                            const int16_t *coefs, uint8_t *out, size_t cap, size_t *out_len);
/* hvc_huffman_optimal_tables over the symbols of the scan as coded with the interval. */
HVC_API int hvc_huffman_optimal_tables_restart(const hvc_jpeg_info *info, const int16_t *coefs, int restart_interval,
                                               hvc_huff_spec out[4]);
/* hvc_huffman_encode_frames (tables = HVC_HUFF_DEFAULT; specs is not read) or hvc_huffman_encode_frames_optimised
 * (HVC_HUFF_OPTIMISED; specs receives n_frames x 4 entries) with the interval: the k_*_rst passes of csrc/hvc_huff.hip.
 * The segments, markers included, equal hvc_jpeg_entropy_encode_restart's.  A frame's unstuffed segment has to stay below
 * 2^29 bytes with its pad bits counted (HVC_E_TOO_LARGE). */
HVC_API int hvc_huffman_encode_frames_restart(hvc_ctx *ctx, const hvc_jpeg_info *info, const int16_t *coefs,
                                              size_t coef_frame_stride, int n_frames, int restart_interval, int tables,
                                              uint8_t *out, size_t out_cap, uint64_t *offsets, hvc_huff_spec *specs,
                                              int where);

/* The same for a batch of equally sized frames (BASELINE config 5 end to end): frames[f] is one raw
 * planar frame as `model encode frame` reads it (Frame.input, common/src/frame.ml:72-76: the tight Y, U,
 * V planes back to back); jpegs[f] receives the file (capacity caps[f]; its length in sizes[f]), byte-
 * identical to Encoder.encode_420/422/444.  Host threads pad planes into a pinned ring, hipMemcpyAsync on a
 * copy stream, the forward block stage and the download of the coefficient records on the compute
 * stream, host threads RLE + Huffman -- three chunks in flight. */
HVC_API int hvc_jpeg_encode_batch(hvc_ctx *ctx, const uint8_t *const *frames, int n_frames, int width, int height,
                                  int chroma, int quality, int threads, int frames_per_chunk,
                                  uint8_t *const *jpegs, const size_t *caps, size_t *sizes,
                                  hvc_batch_stats *stats);
/* The same with the Huffman coder on the GPU as well (hvc_huffman_encode_frames): the coefficient records
 * never leave the device, only the packed entropy-coded segments come back (about 1/6 of the bytes), and
 * the host threads just pad planes and assemble header + segment + EOI.  Same files, byte for byte.
 * HVC_E_TOO_LARGE if a chunk's segments exceed twice the size of its raw frames (use the host-coder
 * variant for such content); stats->coef_bytes then counts the segment bytes downloaded. */
HVC_API int hvc_jpeg_encode_batch_gpu(hvc_ctx *ctx, const uint8_t *const *frames, int n_frames, int width,
                                      int height, int chroma, int quality, int threads, int frames_per_chunk,
                                      uint8_t *const *jpegs, const size_t *caps, size_t *sizes,
                                      hvc_batch_stats *stats);

/* ------------------------------------------------------------------------- */
/* RGB (an extension: the model never upsamples and never converts; csrc/hvc_rgb.hip).  "The RGB image of a file" is
 *   1. the block stage's decoded planes, as hvc_decode_frames writes them, under whichever arithmetic hvc_set_arithmetic
 *      names (the colour pass is a pass of its own, so unlike the fused 4:4:4 path it takes the Hardcaml setting as well);
 *   2. full-size chroma as `oyuv convert ... 444` makes it: Planar_444.supersample_hv2 (4:2:0), supersample_h2 (4:2:2),
 *      nothing (4:4:4) -- the arithmetic of hvc_upsample420 / hvc_upsample422 -- of the top-left chroma_w x chroma_h window
 *      of the chroma planes, chroma_w = ceil(width / 2) (4:2:0, 4:2:2), chroma_h = ceil(height / 2) (4:2:0); the last column
 *      and row of THAT WINDOW are the ones repeated, and the top-left width x height of the result is used.  For even sizes
 *      this is hvc_decode_frames_yuv444's frame; odd sizes use the one extra chroma column / row the decoded plane holds
 *      (under HVC_ARITH_LIBJPEG the filter over that window is libjpeg's: "Bit-exact to libjpeg" below);
 *   3. libjpeg's 16-bit fixed-point form of the JFIF matrix (ITU-T T.871), >> arithmetic, cb = Cb - 128, cr = Cr - 128:
 *          R = clamp(Y + ((  91881 * cr              + 32768) >> 16))
 *          G = clamp(Y + (( -22554 * cb - 46802 * cr + 32768) >> 16))
 *          B = clamp(Y + (( 116130 * cb              + 32768) >> 16))              clamp = to 0 .. 255
 *      and the way back (every output is in 0 .. 255 for every input: no clamp)
 *          Y  = ( 19595 * R + 38470 * G +  7471 * B               + 32768) >> 16
 *          Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
 *          Cr = ( 32768 * R - 27439 * G -  5329 * B + (128 << 16) + 32767) >> 16
 *      followed by Planar_444.subsample_hv2 (4:2:0) / subsample_h2 (4:2:2) of the full-size Cb and Cr planes (the arithmetic
 *      of hvc_subsample420 / hvc_subsample422).  A one-component file is grey: R = G = B = Y.
 * Steps 2 and 3 are one kernel in either direction; the full-size chroma planes exist in registers only.  tools/rgb_reference.py
 * is the same definition in numpy.  Three components are ALWAYS read as Y, Cb, Cr: no Adobe APP14 transform flag, no CMYK.
 *
 * Layouts: HVC_RGB_INTERLEAVED is R G B R G B ..., 3 bytes per pixel ([H, W, 3]); HVC_RGB_PLANAR three width x height planes
 * R, G, B ([3, H, W]).  rgb_row_stride: bytes per row (>= 3 * width interleaved, >= width planar; 0 = tight); planar planes
 * are rgb_row_stride * height apart; rgb_frame_stride: bytes from frame to frame (0 = tight).  Bytes between rows and frames
 * are never written.  `sampling` is HVC_YUV_420 / 422 / 444 or HVC_YUV_400 (luma only: comps[0] alone is read or written);
 * hvc_yuv_frame_bytes and hvc_yuv_convert keep refusing HVC_YUV_400.  `where`, streams and staging as everywhere else
 * (HVC_MEM_DEVICE: enqueued on ctx's stream, returns at once; host memory goes through context scratch and the call blocks).
 * A width, height or n_frames of 0: HVC_OK, nothing written.
 *
 * hvc_yuv_to_rgb      steps 2 + 3 on planes that are already there (pixel records of hvc_decode_frames, or raw frames):
 *                     comps[i].plane_offset / .stride place the planes of frame f at yuv + f * yuv_frame_stride, chroma_w x
 *                     chroma_h are the valid chroma samples.  HVC_E_INVALID_ARG unless 2 * chroma_w >= width (4:4:4: chroma_w
 *                     >= width), 2 * chroma_h >= height for 4:2:0 (else chroma_h >= height), every stride holds its window,
 *                     and (components that name their blocks) the window lies inside blocks_w * 8 x blocks_h * 8.
 * hvc_rgb_to_yuv      the way back into planes at the offsets and strides of comps (the encoder's padded pixel record, or a
 *                     raw frame); only the frame's own samples are written, padding stays the caller's.  Keeps the encoder's
 *                     rule: even width for 4:2:2 and 4:2:0, even height for 4:2:0 (Yuv.assert_is_420 / _422), else
 *                     HVC_E_INVALID_ARG.
 * hvc_decode_frames_rgb  coefficient records -> RGB: hvc_decode_frames into context scratch (tight planes; comps' blocks_w,
 *                     blocks_h, qtab and coef_offset are used, plane_offset / stride ignored), then the colour pass with
 *                     chroma_w = ceil(width / 2) ...; the planes never leave the GPU.  n_comp is 3 (1 for HVC_YUV_400);
 *                     the windows must lie inside the decoded planes.  Honours hvc_set_arithmetic and hvc_set_decode_kernel;
 *                     hvc_last_wide_blocks counts as after hvc_decode_frames.
 * hvc_jpeg_decode_rgb    hvc_jpeg_decode + colour, one file, host memory: rgb receives the image (rgb_cap >= its bytes).
 *                     The sampling follows from the RATIOS of the scan's sampling factors: three components, luma twice the
 *                     chroma both ways -> 4:2:0, in width only -> 4:2:2, all equal -> 4:4:4, one component -> grey.  Anything
 *                     else (4:1:1, 4:4:0, two or four components): HVC_E_INVALID_ARG, output untouched.  Honours
 *                     hvc_set_arithmetic, hvc_set_restart_markers and hvc_set_decode_kernel; blocks that go through the int64
 *                     fix-up and DCs beyond int16 come out as the model's pixels, as in hvc_jpeg_decode.
 * hvc_jpeg_decode_batch_rgb  a batch of files of one geometry: hvc_jpeg_decode_batch (gpu_reader = 0) or
 *                     hvc_jpeg_decode_batch_gpu (gpu_reader != 0) with its planes in context scratch, and the colour pass from
 *                     there to rgb (host or device) on the same stream.  The pipelines run unchanged; the colour pass follows a
 *                     PART of the batch (at most ~4 GB of planes, i.e. some 1300 frames of 1080p), not each ring chunk, so the
 *                     scratch is a part's planes.  stats: the pipelines' sums over the parts; wall_ms includes the colour pass.
 * hvc_jpeg_encode_rgb    hvc_jpeg_encode of the converted planes, byte for byte (chroma 420, 422 or 444; a monochrome encoder
 *                     stays out of scope); honours hvc_set_huffman_tables, hvc_set_restart_interval and
 *                     hvc_set_encode_arithmetic.  The image is uploaded as it is and converted on the GPU.
 * Parameter lists are the issue's; none was adjusted. */
enum { HVC_YUV_400 = 400 }; /* luma only; beside HVC_YUV_420 / 422 / 444 */
typedef enum { HVC_RGB_INTERLEAVED = 0, HVC_RGB_PLANAR = 1 } hvc_rgb_layout;
HVC_API int hvc_yuv_to_rgb(hvc_ctx *ctx, const uint8_t *yuv, size_t yuv_frame_stride, const hvc_component *comps, int sampling,
                           int width, int height, int chroma_w, int chroma_h, int n_frames, uint8_t *rgb,
                           size_t rgb_row_stride, size_t rgb_frame_stride, int layout, int where);
HVC_API int hvc_rgb_to_yuv(hvc_ctx *ctx, const uint8_t *rgb, size_t rgb_row_stride, size_t rgb_frame_stride, int layout,
                           int width, int height, int sampling, int n_frames, uint8_t *yuv, size_t yuv_frame_stride,
                           const hvc_component *comps, int where);
HVC_API int hvc_decode_frames_rgb(hvc_ctx *ctx, const int16_t *coefs, size_t coef_frame_stride, const uint16_t *qtabs,
                                  int n_qtabs, const hvc_component *comps, int n_comp, int sampling, int n_frames, int width,
                                  int height, uint8_t *rgb, size_t rgb_row_stride, size_t rgb_frame_stride, int layout,
                                  int where);
HVC_API int hvc_jpeg_decode_rgb(hvc_ctx *ctx, const uint8_t *jpeg, size_t n, hvc_jpeg_info *info, uint8_t *rgb,
                                size_t rgb_cap, size_t rgb_row_stride, int layout);
HVC_API int hvc_jpeg_decode_batch_rgb(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_frames,
                                      int threads, int frames_per_chunk, int gpu_reader, uint8_t *rgb,
                                      size_t rgb_row_stride, size_t rgb_frame_stride, int layout, int where,
                                      hvc_batch_stats *stats);
HVC_API int hvc_jpeg_encode_rgb(hvc_ctx *ctx, const uint8_t *rgb, size_t rgb_row_stride, int layout, int width, int height,
                                int chroma, int quality, uint8_t *out, size_t cap, size_t *out_len);

/* ------------------------------------------------------------------------- */
/* Bit-exact to libjpeg (an EXTENSION; csrc/hvc_libjpeg.hip): hvc_set_arithmetic(ctx, HVC_ARITH_LIBJPEG) makes the decode
 * entry points compute what libjpeg / libjpeg-turbo compute at their defaults -- the pixels of Pillow, OpenCV, torchvision
 * and djpeg -- instead of the model's.  Two things change: the block stage's inverse DCT, and, in the RGB image of a file,
 * how chroma is brought to full size.  tools/libjpeg_reference.py restates both in numpy; tests/test_libjpeg_reference.py
 * holds that against libjpeg-turbo with 0 mismatches.
 *
 * Block stage: jidctint.c ("islow").  d[k] = coefficient * table entry at natural position k = 8 * row + col; all arithmetic
 * in unbounded integers; D(x, n) = (x + 2^(n-1)) >> n with an arithmetic shift.  One step on v[0..7] with shift sh:
 *     z1 = (v2 + v6) * 4433;  tmp2 = z1 - v6 * 15137;  tmp3 = z1 + v2 * 6270
 *     tmp0 = (v0 + v4) << 13;  tmp1 = (v0 - v4) << 13
 *     t10 = tmp0 + tmp3;  t13 = tmp0 - tmp3;  t11 = tmp1 + tmp2;  t12 = tmp1 - tmp2
 *     a0 = v7; a1 = v5; a2 = v3; a3 = v1
 *     z1 = a0 + a3;  z2 = a1 + a2;  z3 = a0 + a2;  z4 = a1 + a3;  z5 = (z3 + z4) * 9633
 *     a0 *= 2446;  a1 *= 16819;  a2 *= 25172;  a3 *= 12299
 *     z1 *= -7373;  z2 *= -20995;  z3 = z3 * (-16069) + z5;  z4 = z4 * (-3196) + z5
 *     a0 += z1 + z3;  a1 += z2 + z4;  a2 += z2 + z3;  a3 += z1 + z4
 *     D(t10 + a3, sh), D(t11 + a2, sh), D(t12 + a1, sh), D(t13 + a0, sh), D(t13 - a0, sh), D(t12 - a1, sh), D(t11 - a2, sh), D(t10 - a3, sh)
 * Pass 1 runs down the eight columns with sh = 11, pass 2 along the eight rows of the workspace with sh = 18; the sample is
 * clamp(x + 128, 0, 255).  libjpeg's shortcut for a column without AC terms gives the same values and needs no case of its
 * own.  libjpeg-turbo's SIMD code keeps 16-bit intermediates that WRAP for blocks whose pass-1 workspace goes far beyond
 * any real image's (observed around 20 000: every coefficient +-8 with table entries up to 255); as with the range-limit
 * table of jidctred.c in the next section, the definition is the formula, not the wrap.
 * The GPU computes blocks with SUM |d[k]| <= 14000 in int32 and the others in int64 in the same kernel (hvc_last_wide_blocks
 * counts the latter; csrc/hvc_islow_spec.h holds the operation list and the guard, tests/test_islow_guard.py its proof); both
 * give the definition's value for every int16 coefficient and every 16-bit table entry.  hvc_set_decode_kernel has no
 * effect under LIBJPEG, except that 2 sends every block down the int64 path (hvc_last_wide_blocks then reports all of them).
 *
 * Chroma to full size (step 2 of the RGB section above, under LIBJPEG only; steps 1 and 3 and everything else of step 2 --
 * the top-left chroma_w x chroma_h window, ITS edges being the ones repeated, the top-left width x height of the result
 * being used -- are unchanged): libjpeg's "fancy" triangle filter.  With s the window, cw = chroma_w, ch = chroma_h:
 *   4:2:2, cw > 2   out[2i] = (3 s[i] + s[i-1] + 1) >> 2,  out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2,
 *                   except out[0] = s[0] and out[2 cw - 1] = s[cw - 1]
 *   4:2:0, cw > 2   vertically first, unrounded: t[2r] = 3 s[r] + s[max(r-1, 0)],  t[2r+1] = 3 s[r] + s[min(r+1, ch-1)];
 *                   then along each row: out[2i] = (3 t[i] + t[i-1] + 8) >> 4,  out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4,
 *                   except out[0] = (4 t[0] + 8) >> 4 and out[2 cw - 1] = (4 t[cw-1] + 7) >> 4
 *   cw <= 2         (images at most 4 pixels wide) every chroma sample replicated, 2 x or 2 x 2: libjpeg chooses its plain
 *                   routine there
 *   4:4:4, grey     unchanged.
 *
 * Where it applies: hvc_dequant_idct_recon, hvc_decode_frames (host and device memory), hvc_decode_frames_submit,
 * hvc_jpeg_decode, hvc_jpeg_decode_batch, hvc_jpeg_decode_batch_gpu, hvc_yuv_to_rgb, hvc_decode_frames_rgb,
 * hvc_jpeg_decode_rgb and hvc_jpeg_decode_batch_rgb; hvc_set_restart_markers is honoured as before.  A file with a block
 * whose absolute DC does not fit int16 is HVC_E_RANGE (as at the reduced scales: no side list of such blocks).  The fused
 * 4:4:4 and scaled (scale_denom > 1) entry points refuse any arithmetic but MODEL with HVC_E_INVALID_ARG, output untouched,
 * as they do for HARDCAML: their libjpeg forms are not built.  The mixed entry points refuse it under hvc_set_arithmetic in
 * the same way, and have the libjpeg form at full size under a setting of their own (next paragraph).
 * hvc_decode_frames_divergence is unaffected.  hvc_set_encode_arithmetic refuses the value: the encoder side is a setting of
 * its own, hvc_set_encode_libjpeg ("Encoding bit-exact to libjpeg" below).
 *
 * Mixed batches (csrc/hvc_mixed_libjpeg.hip): hvc_set_mixed_arithmetic(ctx, HVC_ARITH_LIBJPEG) gives the mixed decode calls --
 * hvc_decode_frames_mixed, hvc_yuv_to_rgb_mixed, hvc_decode_frames_mixed_rgb, hvc_jpeg_decode_batch_mixed, _mixed_rgb and
 * _mixed_resized with scale_denom 1 -- the two definitions above: the block stage is k_islow_mixed, k_islow's block code under
 * k_decode_mixed's decomposition with the int64 path in the same lane (hvc_last_wide_blocks counts it;
 * hvc_set_decode_kernel(ctx, 2) sends every block there), and the colour pass is k_ycc_to_rgb_fancy_mixed.  Every record is
 * what hvc_jpeg_decode / hvc_jpeg_decode_rgb write for that file alone under hvc_set_arithmetic(ctx, HVC_ARITH_LIBJPEG), with
 * host or device memory and with either mixed reader; hvc_jpeg_decode_batch_mixed_resized then ends in the bytes of Pillow's
 * Image.open(f).convert("RGB").resize((W, H), filter).  The setting is per context, HVC_ARITH_MODEL by default; any other
 * value, HVC_ARITH_HARDCAML included, is HVC_E_INVALID_ARG and leaves the setting as it was.  At the default the mixed calls
 * do what they do without it, refusing any hvc_set_arithmetic but MODEL included; under HVC_ARITH_LIBJPEG they do not look
 * at hvc_set_arithmetic at all.  The reduced-size forms (hvc_decode_frames_mixed_scaled, hvc_jpeg_decode_batch_mixed_scaled,
 * _mixed_scaled_rgb, and _mixed_resized with scale_denom > 1) return HVC_E_INVALID_ARG under it, output untouched: libjpeg
 * decodes the chroma of a subsampled file at another size there, a different definition.  hvc_rgb_resize_mixed and the encode
 * calls take no part in the setting. */
HVC_API int hvc_set_mixed_arithmetic(hvc_ctx *ctx, int arith); /* HVC_ARITH_MODEL (default) | HVC_ARITH_LIBJPEG */
HVC_API int hvc_get_mixed_arithmetic(const hvc_ctx *ctx, int *arith);

/* ------------------------------------------------------------------------- */
/* Encoding bit-exact to libjpeg (an EXTENSION; csrc/hvc_libjpeg_encode.hip): hvc_set_encode_libjpeg(ctx, 1) makes the encode
 * entry points produce the coefficients libjpeg-turbo's compressor writes at its defaults (JDCT_ISLOW, no smoothing,
 * baseline), which is what Pillow, OpenCV and torchvision write.  The claim is about COEFFICIENTS, not file bytes: for the
 * same component samples and the same quantiser tables the coefficient record equals, block for block and dummy blocks
 * included, what libjpeg-turbo puts into its file.  Headers, Huffman tables and the quality-to-table mapping stay this
 * library's (hvc_quant_table and the infos give the tables; a caller who wants Pillow's tables passes them).  The definition
 * is restated in numpy in tools/libjpeg_encode_reference.py; tests/test_libjpeg_encode_reference.py holds that against Pillow
 * (libjpeg-turbo) itself, 0 mismatching coefficients, and tests/golden/libjpeg_encode_pins.json pins Pillow's records.
 *
 * 1. Forward DCT: jfdctint.c's jpeg_fdct_islow on p - 128, CONST_BITS 13 and PASS1_BITS 2, rows first and then columns, the
 *    output t scaled by 8.  The operation list is data, csrc/hvc_fdct_islow_spec.h: the kernel, the numpy form and the
 *    overflow proof (tests/test_fdct_islow_bounds.py: int32 never wraps, every multiplicand fits 24 bits, |t| <= 8192) expand
 *    that one list.
 * 2. Quantiser: with q the table entry and d = 8 q, the value is sign(t) * ((|t| + d / 2) / d) in integer division
 *    (jcdctmgr.c), stored at the entry's zig-zag position, the DC absolute as the records keep it.  Tables are validated as
 *    before (1..255, else HVC_E_RANGE).  The division is one host-made multiplier per entry (csrc/hvc_libjpeg_encode_plan.cpp),
 *    exhausted against C's / for every q and every |t| up to the proved bound (tests/test_libjpeg_encode_plan.py).
 * 3. Edges, where a call knows the frame's size (the file-level calls, and hvc_encode_frames_mixed through its infos' comp[i]
 *    .actual_width / .actual_height): every component, actual_width x actual_height of its info, is repeated to the right and
 *    downward (last column, last row) where the model pads with zeros -- by the file-level calls, which pad; hvc_encode_frames_mixed
 *    reads the padded pixel records it is given, so the samples of a ragged last block are the caller's.  Every block of
 *    the padded layout past the component's own ceil(actual / 8) blocks in either direction is a DUMMY block: its AC
 *    coefficients are 0 and its DC is that of the block before it in libjpeg's MCU buffer (jccoefct.c compress_data),
 *    row-major inside the component's h x v blocks of the MCU -- a dummy in a real row takes the block on its left; every
 *    block of a dummy row takes the LAST block of the row above it in the MCU; both chain through dummies to a real block.
 *    hvc_fdct_quant, hvc_encode_frames and hvc_encode_frames_submit take a layout without sizes: they treat every block as
 *    real and read the samples they are given; so does hvc_encode_frames_mixed for a component whose info states no size
 *    (actual_width or actual_height <= 0).  A stated size whose blocks are not inside the plane is HVC_E_INVALID_ARG.
 *    This library's 4:2:2 files carry the model's sampling factors 2x2 / 1x2 / 1x2 (Parameters.c422), libjpeg's own are
 *    2x1 / 1x1 / 1x1: the same planes and, where the height is a whole number of 16-row MCUs, the same record; elsewhere the
 *    model's layout has one more block row per plane, all dummies, which follow the rule above with the file's own factors.
 *    In the calls that take planes the component planes are the caller's: this library's 4:2:0 / 4:2:2 frames carry chroma
 *    planes of width / 2 (and height / 2), and those are the samples the claim is about.
 * 4. From RGB (hvc_rgb_to_yuv, hvc_jpeg_encode_rgb and the mixed RGB calls): the colour step is the existing libjpeg form
 *    (tools/rgb_reference.py), then jcsample.c's averaging of the full-size chroma -- h2v2: (a + b + c + d + bias) >> 2 with
 *    bias 1, 2, 1, 2, ... along the output row; h2v1: (a + b + bias) >> 1 with bias 0, 1, 0, 1, ... .  Edges: the last column of
 *    the full-size chroma is repeated to whole blocks of the sub-sampled plane BEFORE the averaging (the bias alternates, so a
 *    padded chroma column is not always the copy of the last real one), and the last AVERAGED row is repeated downward
 *    (jcprepct.c); luma is repeated as in 3.  Odd sizes under 4:2:0 / 4:2:2 stay refused as before.  k_rgb_to_ycc_libjpeg and
 *    k_rgb_to_ycc_libjpeg_mixed expand one lane (csrc/hvc_rgb_libjpeg_dev.h) that works in the coordinates of the output planes
 *    and clamps what it reads: in the encode pipelines (hvc_jpeg_encode_rgb, hvc_encode_frames_mixed_rgb,
 *    hvc_jpeg_encode_batch_mixed_rgb[_gpu]) the colour pass itself writes every component up to ceil(actual / 8) * 8 both ways
 *    -- the pipelines' clear of the plane slot stays, what lies beyond are dummy blocks -- while hvc_rgb_to_yuv and
 *    hvc_rgb_to_yuv_mixed write the frame's own samples and nothing else, as without the setting.
 *
 * Where it applies.  The setting is per context, 0 by default, independent of every other setting; at 0 every entry point
 * does byte for byte what it does without it.  At 1 hvc_set_encode_arithmetic is not consulted, except that HVC_ARITH_HARDCAML
 * together with it is HVC_E_INVALID_ARG at the encode call, output untouched.  It applies to hvc_fdct_quant, hvc_encode_frames
 * (host and device memory), hvc_encode_frames_submit, hvc_jpeg_encode, hvc_jpeg_encode_batch and hvc_jpeg_encode_batch_gpu:
 * k_fdct_islow in k_encode's launch geometry and record layout, and behind it on the same stream k_dummy_blocks for the
 * file-level calls; and to hvc_encode_frames_mixed, hvc_jpeg_encode_batch_mixed and hvc_jpeg_encode_batch_mixed_gpu:
 * k_fdct_islow_mixed under k_encode_mixed's decomposition, its multipliers a record per distinct table and the dummy blocks a
 * list of (record, source) pairs beside the plan image, uploaded only under the setting, k_dummy_blocks_mixed behind it.  Every
 * file of a mixed call is what hvc_jpeg_encode writes for that frame alone under the setting; statuses are as before.  The
 * Huffman coders sit behind the records and do not change; hvc_set_huffman_tables and hvc_set_restart_interval combine with it.
 * From RGB it applies to hvc_rgb_to_yuv, hvc_jpeg_encode_rgb, hvc_rgb_to_yuv_mixed, hvc_encode_frames_mixed_rgb,
 * hvc_jpeg_encode_batch_mixed_rgb and hvc_jpeg_encode_batch_mixed_rgb_gpu (4. above); every file of the mixed RGB calls is what
 * hvc_jpeg_encode_rgb writes for that image alone under the setting.
 * Refused under the setting with HVC_E_INVALID_ARG, output untouched, never computed the model's way in silence:
 *   hvc_encode_frames_recon, hvc_encode_frames_divergence                         (no libjpeg form)
 * hvc_set_encode_libjpeg: HVC_E_INVALID_ARG for anything but 0 and 1, the setting unchanged. */
HVC_API int hvc_set_encode_libjpeg(hvc_ctx *ctx, int on);      /* 0 (default) | 1 */
HVC_API int hvc_get_encode_libjpeg(const hvc_ctx *ctx, int *on);

/* ------------------------------------------------------------------------- */
/* Decoding at reduced size: 1/2, 1/4, 1/8 (an EXTENSION; the model has no counterpart).  libjpeg's scale_denom: the inverse
 * DCT produces N x N samples per block, N = 8 / scale_denom, straight from the coefficients -- the arithmetic of libjpeg's
 * jidctred.c, bit for bit (tools/scaled_reference.py restates it in numpy and tests/test_scaled_reference.py holds that
 * against libjpeg-turbo).  scale_denom s in {1, 2, 4, 8}; for a block d[k] = coefficient * table entry at natural position
 * k = 8 * row + col; all arithmetic in unbounded integers; D(x, n) = (x + 2^(n-1)) >> n with an arithmetic shift; a sample
 * is clamp(x + 128, 0, 255).
 *   N = 1   x = D(d[0], 3).
 *   N = 2   step on v[0..7]:  t10 = v0 << 15;  t0 = -5906 v7 + 6967 v5 - 10426 v3 + 29692 v1;  D(t10 + t0, sh), D(t10 - t0, sh).
 *           Pass 1 down columns 0 1 3 5 7 with sh = 13 (columns 2 4 6 are not used), pass 2 along the two rows of the
 *           workspace with sh = 20.
 *   N = 4   t0 = v0 << 14;  t2 = 15137 v2 - 6270 v6;  t10 = t0 + t2;  t12 = t0 - t2;
 *           o0 = -1730 v7 + 11893 v5 - 17799 v3 + 8697 v1;  o2 = -4176 v7 - 4926 v5 + 7373 v3 + 20995 v1;
 *           D(t10 + o2, sh), D(t12 + o0, sh), D(t12 - o0, sh), D(t10 - o2, sh).  Pass 1 down columns 0 1 2 3 5 6 7 with sh = 12
 *           (column 4 is not used), pass 2 along the four rows with sh = 19.
 *   s = 1   the model's arithmetic, unchanged: the existing entry points.
 * libjpeg's shortcut for a column without AC terms gives the same values and needs no case of its own; where libjpeg limits
 * the range through a masked table (which wraps for absurd inputs) the definition here is the clamp.  EVERY component is
 * scaled by the same s: a decoded plane of blocks_w * 8 x blocks_h * 8 samples becomes blocks_w * N x blocks_h * N.  This is
 * NOT what libjpeg does with a subsampled file, where it decodes the chroma planes at a larger N in place of upsampling
 * them: here a 4:2:0 file at s = 2 gives 4:2:0 planes of half the size, and the RGB form upsamples those.
 * The GPU computes blocks within a proven bound in int32 and the others in int64 in the same kernel (hvc_last_wide_blocks
 * counts the latter); both give the definition's value for every int16 coefficient and every 16-bit table entry.
 * There is no Hardcaml RTL form: with HVC_ARITH_HARDCAML set, the entry points below return HVC_E_INVALID_ARG for s > 1 and
 * leave their output untouched.  Any other scale_denom is HVC_E_INVALID_ARG.
 *
 * hvc_jpeg_scaled_info (host only): *out = *info at 1/s: width, height and every actual_* become ceil(x * N / 8), every
 *   decoded_* becomes x * N / 8; the layout is tight (stride = blocks_w * N, planes back to back) and pixel_bytes its size;
 *   tables, coef_count and the coefficient offsets are unchanged, layout[].blocks_* stay in blocks.
 * hvc_decode_frames_scaled: hvc_decode_frames whose comps[].plane_offset / .stride describe the scaled planes.  These accept
 *   any stride >= blocks_w * N, any plane_offset and any pixel_frame_stride >= the record's span (rows that all start on
 *   4-byte boundaries are written as dwords, others byte by byte); the coefficients' alignment rules are hvc_decode_frames'.
 *   s = 1 is hvc_decode_frames with all its rules.  A device-memory call honours hvc_set_profiling.
 * hvc_jpeg_decode_scaled: one file, read on the host; *info receives the scaled info, pixels (pixel_cap >= its pixel_bytes)
 *   the scaled padded planes.  Honours hvc_set_restart_markers.  At s > 1 a file with a block whose absolute DC does not
 *   fit int16 is HVC_E_RANGE here and in the two below (as for the entry points that return records: the scaled block stage
 *   keeps no side list of such blocks).  s = 1 is hvc_jpeg_decode / hvc_jpeg_decode_rgb / the full-size batch pipelines
 *   themselves, which decode such a file as the model does.
 * hvc_jpeg_decode_scaled_rgb: the same, then the JFIF colour conversion of hvc_jpeg_decode_rgb over the scaled info's width
 *   x height; samplings and refusals as there.
 * hvc_jpeg_decode_batch_scaled: hvc_jpeg_decode_batch (gpu_reader = 0) or hvc_jpeg_decode_batch_gpu (gpu_reader != 0) with
 *   the scaled block stage per chunk; frames are scaled records pixel_frame_stride >= pixel_bytes apart.  Full-size planes
 *   exist nowhere; behind the GPU reader the 1/8 decode reads nothing but the compact DC array.  With hvc_set_profiling on,
 *   the scaled block stage of every chunk (s > 1) takes an entry of the ring: hvc_kernel_ms_history(n = chunks) after the
 *   call holds k_decode_scaled's time per chunk (the full-size pipelines take none). */
HVC_API int hvc_jpeg_scaled_info(const hvc_jpeg_info *info, int scale_denom, hvc_jpeg_info *out);
HVC_API int hvc_decode_frames_scaled(hvc_ctx *ctx, const int16_t *coefs, size_t coef_frame_stride, const uint16_t *qtabs,
                                     int n_qtabs, const hvc_component *comps, int n_comp, int n_frames, int scale_denom,
                                     uint8_t *pixels, size_t pixel_frame_stride, int where);
HVC_API int hvc_jpeg_decode_scaled(hvc_ctx *ctx, const uint8_t *jpeg, size_t n, int scale_denom, hvc_jpeg_info *info,
                                   uint8_t *pixels, size_t pixel_cap);
HVC_API int hvc_jpeg_decode_scaled_rgb(hvc_ctx *ctx, const uint8_t *jpeg, size_t n, int scale_denom, hvc_jpeg_info *info,
                                       uint8_t *rgb, size_t rgb_cap, size_t rgb_row_stride, int layout);
HVC_API int hvc_jpeg_decode_batch_scaled(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_frames,
                                         int threads, int frames_per_chunk, int gpu_reader, int scale_denom, uint8_t *pixels,
                                         size_t pixel_frame_stride, int where, hvc_batch_stats *stats);

/* ------------------------------------------------------------------------- */
/* Mixed batches: frames and files of DIFFERENT sizes, samplings and quantiser tables in one call.  Every other batch entry
 * point takes one geometry and one set of tables and refuses a file that differs from the first (and still does); a directory
 * of photographs has as many geometries as files.  Here the block stage takes its work decomposition from tables in device
 * memory (k_decode_mixed): a launch serves any set of planes, a 64 x 64 thumbnail costs three wavefronts.  The output is
 * full-size padded planes, or RGB images (below: hvc_jpeg_mixed_rgb_layout, hvc_yuv_to_rgb_mixed, hvc_decode_frames_mixed_rgb,
 * hvc_jpeg_decode_batch_mixed_rgb, whose colour pass k_ycc_to_rgb_mixed takes its decomposition from device memory the same
 * way), or either at 1/2, 1/4, 1/8 size (further below: the *_mixed_scaled* entry points, block stage k_decode_mixed_scaled);
 * there is no 4:4:4-planar form and no side list of DCs beyond int16; the files are read by the host Huffman reader or, with
 * hvc_set_mixed_reader(ctx, HVC_READER_GPU), by the mixed GPU Huffman reader (further below).  With
 * HVC_ARITH_HARDCAML set the ctx functions return HVC_E_INVALID_ARG; hvc_set_decode_kernel(ctx, 2) sends every block
 * through the int64 arithmetic, other selections are ignored; hvc_last_wide_blocks counts the blocks that took it.
 * hvc_set_mixed_arithmetic(ctx, HVC_ARITH_LIBJPEG) ("Bit-exact to libjpeg" above) makes the full-size calls of this section
 * and of the RGB and resized ones below compute libjpeg's pixels instead (k_islow_mixed, k_ycc_to_rgb_fancy_mixed) and the
 * reduced-size ones return HVC_E_INVALID_ARG; it replaces what hvc_set_arithmetic says for these calls, which is otherwise
 * honoured as stated here. */

/* headers of n_files files -> infos[f], status[f] (what hvc_jpeg_read_header returns for file f),
 * pixel_offsets[f] (bytes; each record = the file's padded planes exactly as hvc_jpeg_decode lays them out,
 * info.pixel_bytes long, records in file order, each start rounded up to `align`), *total_bytes.
 * A file whose status is not HVC_OK takes no room.  align: a power of two >= 8; 0 = 256. */
HVC_API int hvc_jpeg_mixed_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, size_t align,
                                  hvc_jpeg_info *infos, int *status, size_t *pixel_offsets, size_t *total_bytes);

/* The block stage over frames of DIFFERENT geometry and tables in one launch: frame f is infos[f].layout / .qtabs,
 * its coefficient record at coefs + coef_offsets[f] (int16 elements), its pixel record at pixels + pixel_offsets[f].
 * infos/offsets: host memory always.  Same arithmetic and same bytes as hvc_decode_frames frame by frame.
 * Every coefficient plane must start on 16 bytes, every pixel plane and stride on 8 (HVC_E_ALIGNMENT); a component
 * without a block is skipped, a set without a block launches nothing.  HVC_MEM_DEVICE: enqueued on ctx's stream, honours
 * hvc_set_profiling (the pair brackets k_decode_mixed); HVC_MEM_HOST: staged through context scratch, the call blocks. */
HVC_API int hvc_decode_frames_mixed(hvc_ctx *ctx, const int16_t *coefs, const size_t *coef_offsets,
                                    const hvc_jpeg_info *infos, int n_frames, uint8_t *pixels,
                                    const size_t *pixel_offsets, int where);

/* Files -> pixels.  infos / status / pixel_offsets as hvc_jpeg_mixed_layout made them (the caller sized `pixels` from
 * *total_bytes).  Host threads read the files (the host Huffman reader, restart markers honoured when
 * hvc_set_restart_markers says so) into a pinned ring, chunk by chunk; a chunk = consecutive files whose coefficient
 * records fit chunk_bytes (0 = 64 MiB; a single file larger than that is a chunk of its own and the ring grows);
 * upload || hvc_decode_frames_mixed of the previous chunk || reading of the next, as in hvc_jpeg_decode_batch.
 * PER-FILE results: status[f] receives the file's own code; a file that fails (at its header or in its scan) leaves its
 * pixel record untouched and does not stop the others.  The call itself fails only for its own reasons (arguments,
 * HIP, memory, threads).  A file with a block whose absolute DC leaves int16 is HVC_E_RANGE here (no side list, as at
 * the reduced scales).  Host output: the alignment padding between the records of two good files may be overwritten.
 * stats->frames_per_chunk is the largest chunk's file count, stats->coef_bytes the sum uploaded. */
HVC_API int hvc_jpeg_decode_batch_mixed(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_files,
                                        int threads, size_t chunk_bytes, const hvc_jpeg_info *infos, int *status,
                                        const size_t *pixel_offsets, uint8_t *pixels, size_t pixel_cap, int where,
                                        hvc_batch_stats *stats);

/* Which Huffman reader the mixed batch calls use (hvc_jpeg_decode_batch_mixed, _mixed_rgb, _mixed_scaled, _mixed_scaled_rgb).
 * HVC_READER_HOST (the default): host threads read the files, every launch and byte as described above.
 * HVC_READER_GPU: the mixed GPU Huffman reader (csrc/hvc_hdec_mixed.hip) -- hvc_jpeg_entropy_decode_gpu's self-synchronising
 *   reader with everything a lane needs about its file (geometry, place of its segment and of its record, table set) in a
 *   per-file descriptor in device memory, so that one chain of launches serves files of any size, sampling and tables, and
 *   with one verdict per FILE.  Host threads only unstuff the segments into a pinned ring; the reader writes the
 *   coefficient records into the device slot the block stage reads; chunks are cut as above.  A file is handed back to the
 *   host reader when its verdict is not clean (whatever the model raises on, a DC beyond int16, a stream that ends early or
 *   does not fall into step within the reader's fixed number of rounds), when the reader cannot take it (no 1..3 components,
 *   more than 16 blocks per MCU, an MCU grid that leaves a plane, sizes beyond 32-bit indices, tables that are no prefix
 *   code, a table set or segment that does not fit its chunk's slot), or when it carries restart intervals while
 *   hvc_set_restart_markers is on.  The handed-back files go through the host-reader pipeline in one pass behind the GPU
 *   chunks: results and error codes are the host reader's, byte for byte -- which reader ran never changes a result.
 * hvc_last_mixed_reader_files: of the files that reached a reader in the last mixed batch call, how many records the GPU
 *   reader produced and how many the host reader read (either pointer may be NULL). */
#define HVC_READER_HOST 0
#define HVC_READER_GPU 1
HVC_API int hvc_set_mixed_reader(hvc_ctx *ctx, int which);
HVC_API int hvc_get_mixed_reader(const hvc_ctx *ctx, int *which);
HVC_API int hvc_last_mixed_reader_files(const hvc_ctx *ctx, uint64_t *gpu_files, uint64_t *host_files);
/* The mixed counterpart of hvc_jpeg_entropy_decode_gpu: the files' coefficient records exactly as hvc_jpeg_entropy_decode
 * writes them, file f's at coefs + coef_offsets[f] (int16 elements, a multiple of 8: 16 bytes; `where` says where coefs
 * lives; coef_cap elements in all).  infos / status as hvc_jpeg_mixed_layout made them: a file whose status is not HVC_OK
 * is skipped; status[f] receives the file's own code.  used_gpu[f] (optional) = 1 where the GPU reader produced the record;
 * a handed-back file (see hvc_set_mixed_reader) is read by the host reader on the calling thread.  Blocking. */
HVC_API int hvc_jpeg_entropy_decode_gpu_mixed(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_files,
                                              const hvc_jpeg_info *infos, int *status, int16_t *coefs,
                                              const size_t *coef_offsets, size_t coef_cap, int where, int *used_gpu);

/* Mixed batches to RGB: the colour pass of the RGB section above (same definition, byte for byte what hvc_yuv_to_rgb /
 * hvc_decode_frames_rgb / hvc_jpeg_decode_rgb give for each image alone) over images of ANY size and sampling in one launch.
 * Image f is infos[f].width x .height; its sampling follows from infos[f].n_comp and .comp[].hscale / .vscale by the rule of
 * hvc_jpeg_decode_rgb (4:2:0, 4:2:2, 4:4:4, grey; anything else has no RGB image); its chroma window is ceil(width / 2) x
 * ceil(height / 2) (4:2:0) and so on, as in hvc_decode_frames_rgb.  It lies at rgb + rgb_offsets[f] -- any byte offset -- with
 * rows rgb_row_strides[f] bytes apart (>= 3 * width interleaved, >= width planar; an entry of 0, or rgb_row_strides == NULL:
 * tight rows) and planar planes rgb_row_strides[f] * height apart.  One call has one `layout`.  Images whose address and
 * strides are multiples of 8 are written in 8-byte pieces, the others byte by byte: tight interleaved rows qualify only
 * when width % 8 == 0, so row_align = 8 buys the fast path for every width.  A frame with width * height == 0 is skipped.
 * Parameter lists are the issue's; none was adjusted.
 *
 * hvc_jpeg_mixed_rgb_layout (host only): headers as hvc_jpeg_mixed_layout reads them; a file whose header reads but whose
 *   sampling has no RGB image gets status[f] = HVC_E_INVALID_ARG.  A file with a nonzero status takes no room.  A good
 *   file's record is rgb_row_strides[f] * height bytes (planar: * 3), rgb_row_strides[f] = 3 * width (planar: width) rounded
 *   up to row_align; records in file order, each start rounded up to align.  align, row_align: powers of two >= 1
 *   (else HVC_E_INVALID_ARG); align 0 = 256, row_align 0 = 1 (tight rows: what a tensor view wants).
 * hvc_yuv_to_rgb_mixed: the colour pass alone over planes that are already there: frame f's planes at yuv + yuv_offsets[f],
 *   laid out by infos[f].layout (plane_offset, stride; a component that names its blocks must hold the window).
 *   HVC_MEM_DEVICE: one launch, enqueued on ctx's stream, returns at once, honours hvc_set_profiling (the pair brackets
 *   k_ycc_to_rgb_mixed); HVC_MEM_HOST: staged through context scratch, the call blocks.  Bytes between rows and between
 *   records are never written.  HVC_E_INVALID_ARG: a frame whose sampling has no RGB image, a stride below its row, a window
 *   outside its planes; HVC_E_TOO_LARGE: a side above 2^24 or more lanes than the launch can index.
 * hvc_decode_frames_mixed_rgb: hvc_decode_frames_mixed into context scratch (tight records), then the mixed colour pass; the
 *   planes never leave the GPU.  coefs / coef_offsets / alignment rules as there; hvc_last_wide_blocks counts as after
 *   hvc_decode_frames_mixed; a device-memory call honours hvc_set_profiling as that one does (the pair brackets k_decode_mixed).
 * hvc_jpeg_decode_batch_mixed_rgb: hvc_jpeg_decode_batch_mixed's pipeline with the colour pass behind every chunk's block
 *   stage, on the same stream; infos / status / rgb_offsets / rgb_row_strides as hvc_jpeg_mixed_rgb_layout made them.  PER-FILE
 *   results as there: a file that fails at its header, by its sampling (HVC_E_INVALID_ARG) or in its scan leaves its RGB record
 *   untouched and stops nobody; a DC beyond int16 is HVC_E_RANGE.  rgb_cap: bytes of rgb; every good file's image must lie
 *   inside (HVC_E_INVALID_ARG).  Host output: the alignment padding between the records of two good files may be overwritten
 *   (bytes between the rows of an image are not).  stats as hvc_jpeg_decode_batch_mixed; kernel_ms_sum includes the colour pass. */
HVC_API int hvc_jpeg_mixed_rgb_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int layout, size_t align,
                                      size_t row_align, hvc_jpeg_info *infos, int *status, size_t *rgb_offsets,
                                      size_t *rgb_row_strides, size_t *total_bytes);
HVC_API int hvc_yuv_to_rgb_mixed(hvc_ctx *ctx, const uint8_t *yuv, const size_t *yuv_offsets, const hvc_jpeg_info *infos,
                                 int n_frames, uint8_t *rgb, const size_t *rgb_offsets, const size_t *rgb_row_strides,
                                 int layout, int where);
HVC_API int hvc_decode_frames_mixed_rgb(hvc_ctx *ctx, const int16_t *coefs, const size_t *coef_offsets,
                                        const hvc_jpeg_info *infos, int n_frames, uint8_t *rgb, const size_t *rgb_offsets,
                                        const size_t *rgb_row_strides, int layout, int where);
HVC_API int hvc_jpeg_decode_batch_mixed_rgb(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_files,
                                            int threads, size_t chunk_bytes, const hvc_jpeg_info *infos, int *status,
                                            const size_t *rgb_offsets, const size_t *rgb_row_strides, uint8_t *rgb,
                                            size_t rgb_cap, int layout, int where, hvc_batch_stats *stats);

/* Mixed batches at reduced size: thumbnails or previews of a set of files in one call.  scale_denom is 1, 2, 4 or 8 (anything
 * else: HVC_E_INVALID_ARG); 1 IS the full-size entry point of the same name without "_scaled", with all its rules (its 8-byte
 * alignment; scaled[f] == infos[f]).  At 2, 4, 8 the block stage is k_decode_mixed_scaled: the reduced-size inverse DCT of
 * "Decoding at reduced size" above (N = 8 / scale_denom samples per block side, its int32 guard and int64 branch in the same
 * lane) under k_decode_mixed's work decomposition; every byte is what hvc_decode_frames_scaled / hvc_jpeg_decode_scaled[_rgb]
 * give for that frame or file alone.  Full-size planes exist nowhere.  HVC_ARITH_HARDCAML: HVC_E_INVALID_ARG, output untouched.
 * hvc_last_wide_blocks counts the blocks of the int64 branch, as after hvc_decode_frames_scaled; hvc_set_decode_kernel is
 * ignored.  In the file pipelines the host Huffman reader is the bound at every scale: what the scaled form saves is the
 * output's memory and download, not time in the block stage.
 *
 * hvc_jpeg_mixed_scaled_layout (host only): headers -> infos[f] (FULL-size, what hvc_jpeg_read_header gives: the batch call's
 *   input), scaled[f] (hvc_jpeg_scaled_info of it: what describes file f's output record), status[f], pixel_offsets[f],
 *   *total_bytes; records = scaled[f].pixel_bytes, in file order, each start rounded up to align (a power of two >= 8; 0 =
 *   256); a file with a nonzero status takes no room (and its scaled[f] is not written).
 * hvc_decode_frames_mixed_scaled: frame f: infos[f].layout's blocks_w / blocks_h / qtab / coef_offset as ever, .plane_offset /
 *   .stride describe its SCALED planes by hvc_decode_frames_scaled's rule: any offset, any stride >= blocks_w * N (below:
 *   HVC_E_INVALID_ARG); coefficient planes on 16 bytes as ever.  A plane whose first byte and stride are multiples of 4 is
 *   written in dwords, any other in 2-byte / 1-byte pieces (tight strides: blocks_w odd at N = 2, blocks_w % 4 != 0 at N = 1).
 *   Bytes between rows and between records are never written.  HVC_MEM_DEVICE: one launch on ctx's stream, honours
 *   hvc_set_profiling (the pair brackets k_decode_mixed_scaled); HVC_MEM_HOST: staged through context scratch, the call blocks.
 * hvc_jpeg_decode_batch_mixed_scaled: hvc_jpeg_decode_batch_mixed's pipeline, statuses, chunks and stats; infos = the FULL-size
 *   infos of the layout call, records as hvc_jpeg_mixed_scaled_layout placed them (any offset is accepted).  pixel_cap: every
 *   good file's record must lie inside (HVC_E_INVALID_ARG).  Host output: no byte outside the good files' records is written.
 * hvc_jpeg_mixed_scaled_rgb_layout / hvc_jpeg_decode_batch_mixed_scaled_rgb: as hvc_jpeg_mixed_rgb_layout /
 *   hvc_jpeg_decode_batch_mixed_rgb with image f = scaled[f].width x scaled[f].height, byte for byte what
 *   hvc_jpeg_decode_scaled_rgb gives for file f alone; the chunk's scaled planes go to the device plane ring (sized from the
 *   scaled pixel_bytes) and k_ycc_to_rgb_mixed runs from there. */
HVC_API int hvc_jpeg_mixed_scaled_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int scale_denom,
                                         size_t align, hvc_jpeg_info *infos, hvc_jpeg_info *scaled, int *status,
                                         size_t *pixel_offsets, size_t *total_bytes);
HVC_API int hvc_decode_frames_mixed_scaled(hvc_ctx *ctx, const int16_t *coefs, const size_t *coef_offsets,
                                           const hvc_jpeg_info *infos, int n_frames, int scale_denom, uint8_t *pixels,
                                           const size_t *pixel_offsets, int where);
HVC_API int hvc_jpeg_decode_batch_mixed_scaled(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_files,
                                               int threads, size_t chunk_bytes, int scale_denom, const hvc_jpeg_info *infos,
                                               int *status, const size_t *pixel_offsets, uint8_t *pixels, size_t pixel_cap,
                                               int where, hvc_batch_stats *stats);
HVC_API int hvc_jpeg_mixed_scaled_rgb_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int scale_denom,
                                             int layout, size_t align, size_t row_align, hvc_jpeg_info *infos,
                                             hvc_jpeg_info *scaled, int *status, size_t *rgb_offsets,
                                             size_t *rgb_row_strides, size_t *total_bytes);
HVC_API int hvc_jpeg_decode_batch_mixed_scaled_rgb(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_files,
                                                   int threads, size_t chunk_bytes, int scale_denom, const hvc_jpeg_info *infos,
                                                   int *status, const size_t *rgb_offsets, const size_t *rgb_row_strides,
                                                   uint8_t *rgb, size_t rgb_cap, int layout, int where, hvc_batch_stats *stats);

/* ------------------------------------------------------------------------- */
/* Mixed batches, ENCODING: frames of DIFFERENT sizes, samplings and qualities in one call -- what hvc_jpeg_decode_batch_mixed
 * [_scaled] hands back (thumbnails, a photo set to recompress, a dataset rewritten at another quality) made into files again.
 * The forward block stage takes its work decomposition from tables in device memory as the mixed decode does
 * (k_encode_mixed, csrc/hvc_mixed_encode.hip: one wavefront per 64 blocks of one plane, k_encode's arithmetic per block), so
 * every coefficient is what hvc_encode_frames gives for that frame alone and every file what hvc_jpeg_encode gives for it.
 * With HVC_ARITH_HARDCAML as the ENCODE arithmetic (hvc_set_encode_arithmetic) the ctx functions return HVC_E_INVALID_ARG,
 * outputs untouched.  Here the files are coded by host threads (the Huffman coder on the GPU: the next section).  RGB input:
 * the section after that.  Not here: monochrome.
 *
 * hvc_jpeg_encoder_mixed_layout (host only, no ctx): per frame hvc_jpeg_encoder_layout(widths[f], heights[f], chromas[f],
 *   qualities[f]) + hvc_jpeg_encoder_check -> infos[f], status[f] (that frame's own code: a refused frame takes no room and
 *   stops nobody).  A good frame's padded pixel record (info.pixel_bytes) lies at pixel_offsets[f], bytes, each start
 *   rounded up to align (0, or a power of two >= 8; 0 = 64); its coefficient record (info.coef_count) at coef_offsets[f],
 *   int16 elements, each start on 16 bytes.  *pixel_total bytes and *coef_total elements hold all of them.
 * hvc_encode_frames_mixed: frame f is infos[f].layout / .qtabs; its padded planes are read from pixels + pixel_offsets[f],
 *   its coefficient record is written at coefs + coef_offsets[f].  infos / offsets: host memory always.  Every coefficient
 *   plane must start on 16 bytes, every pixel plane and stride on 8 (HVC_E_ALIGNMENT).  HVC_E_INVALID_ARG: a component with
 *   blocks_w or blocks_h of 0 (hvc_component: the encoding entry points refuse it); HVC_E_RANGE: a table entry of 0 or above
 *   255 (the model's encoder tables are 8-bit); nothing is written then.  HVC_MEM_DEVICE: one launch, enqueued on ctx's
 *   stream, returns at once, honours hvc_set_profiling (the pair brackets k_encode_mixed); HVC_MEM_HOST: staged through
 *   context scratch, the call blocks, and only the coefficient planes are copied back (gaps in `coefs` stay untouched).
 *   A set without a frame is HVC_OK and needs no memory.
 * hvc_jpeg_encode_batch_mixed: frames[f] = one raw planar frame as `model encode frame` reads it (tight Y, U, V of
 *   infos[f].width x .height at its sampling); infos / status as the layout call made them: only frames with status[f] ==
 *   HVC_OK take part.  hvc_jpeg_encode_batch's pipeline with chunks cut by the bytes of the frames' padded pixel records
 *   (chunk_bytes 0 = 64 MiB; a frame larger than that is a chunk of its own and the ring grows): host threads pad each frame
 *   into a pinned ring, upload on the copy stream || k_encode_mixed with one plan per chunk || download of the chunk's
 *   records, `threads` host threads code each file with its own info (a quarter as many more do the padding).  Honours
 *   hvc_set_huffman_tables (default, or per-file optimised), hvc_set_restart_interval and hvc_set_host_cpus.  PER-FILE
 *   results: sizes[f] bytes at jpegs[f] for a good file; caps[f] too small: status[f] = HVC_E_INVALID_ARG and sizes[f] = the
 *   size it needs; a value without a Huffman code: HVC_E_RANGE for that file alone; a frame that was refused before the
 *   call keeps its status, jpegs[f] and sizes[f] untouched.  The call's own return value is for what concerns the whole
 *   call (arguments, memory, HIP, threads).  stats as hvc_jpeg_encode_batch; frames_per_chunk = the largest chunk's count. */
HVC_API int hvc_jpeg_encoder_mixed_layout(const int *widths, const int *heights, const int *chromas, const int *qualities,
                                          int n_frames, size_t align, hvc_jpeg_info *infos, int *status,
                                          size_t *pixel_offsets, size_t *coef_offsets, size_t *pixel_total,
                                          size_t *coef_total);
HVC_API int hvc_encode_frames_mixed(hvc_ctx *ctx, const uint8_t *pixels, const size_t *pixel_offsets,
                                    const hvc_jpeg_info *infos, int n_frames, int16_t *coefs, const size_t *coef_offsets,
                                    int where);
HVC_API int hvc_jpeg_encode_batch_mixed(hvc_ctx *ctx, const uint8_t *const *frames, const hvc_jpeg_info *infos, int *status,
                                        int n_frames, int threads, size_t chunk_bytes, uint8_t *const *jpegs,
                                        const size_t *caps, size_t *sizes, hvc_batch_stats *stats);

/* ------------------------------------------------------------------------- */
/* Mixed batches, ENCODING, with the Huffman coder on the GPU: the passes of hvc_huffman_encode_frames with the geometry of
 * every work unit taken from device memory (csrc/hvc_huff_mixed.hip: one wavefront per 64 blocks of one plane of one file, a
 * status word per file), so frames of different sizes and samplings are coded in one chain of launches.  Not in this coder:
 * restart intervals (the batch call hands such calls to the host coder), monochrome, the Hardcaml arithmetic.
 *
 * hvc_huffman_encode_frames_mixed: the coder alone.  Frame f is infos[f]; its coefficient record (as hvc_encode_frames_mixed
 *   writes it) is read from coefs + coef_offsets[f], which must lie on 16 bytes (HVC_E_ALIGNMENT for the call: an offset that
 *   is no multiple of 8 elements; HVC_MEM_DEVICE: coefs off 16 bytes, offsets off 8).  tables = HVC_HUFF_DEFAULT or
 *   HVC_HUFF_OPTIMISED (anything else: HVC_E_INVALID_ARG).  Frame f's entropy-coded segment -- the bytes between the header
 *   and EOI of hvc_jpeg_entropy_encode / hvc_jpeg_entropy_encode_tables for that frame -- is out[offsets[f] .. offsets[f + 1]);
 *   offsets has n_frames + 1 entries, the segments lie back to back.  status[f] is the frame's OWN code, and a frame that is
 *   refused or flagged has an empty segment and stops nobody: hvc_jpeg_encoder_check's refusal (n_comp != 3 among them), a
 *   component without a block or a grid without an MCU (HVC_E_INVALID_ARG), more than 2^32 bits (HVC_E_TOO_LARGE), under
 *   HVC_HUFF_OPTIMISED all components on one table set (HVC_E_INVALID_ARG, as hvc_huffman_optimal_tables), a value without a
 *   code -- a DC difference beyond 11 bits, an AC value beyond 10 -- HVC_E_RANGE.  With HVC_HUFF_OPTIMISED specs (n_frames x 4:
 *   DC0, DC1, AC0, AC1) receives each good frame's tables, equal to hvc_huffman_optimal_tables'; otherwise specs may be NULL.
 *   out_cap smaller than the segments: HVC_E_INVALID_ARG for the call, `out` untouched.  coefs, out and offsets live where
 *   `where` says; infos, coef_offsets, status and specs are host memory always.  The call blocks.  More than 65535 good frames:
 *   HVC_E_TOO_LARGE.  A set without a frame is HVC_OK and needs no memory.
 * hvc_jpeg_encode_batch_mixed_gpu: hvc_jpeg_encode_batch_mixed, argument for argument, with that coder behind k_encode_mixed:
 *   the same files byte for byte, the same status[f] and sizes[f] (caps[f] too small: HVC_E_INVALID_ARG, sizes[f] = the size
 *   needed, jpegs[f] untouched).  Chunks are cut as there, and hold at most 65535 files; a chunk's records stay on the device,
 *   the coder writes its packed segments into a device slot of the size of its records, and only the offsets, the status
 *   words, the specs (optimised tables) and exactly the segments come down (stats->coef_bytes counts the segment bytes);
 *   `threads` host threads put header + segment + EOI together.  Honours hvc_set_huffman_tables and hvc_set_host_cpus.  Files
 *   the GPU path does not finish -- flagged by the length pass, past the segment slot, refused by the coder's plan, and EVERY
 *   file when hvc_set_restart_interval is non-zero -- are coded by the host coder in one pass behind the GPU chunks; which
 *   coder ran never changes a byte, a status or a size.  Measured against the host coder on a seeded set of 4096 frames: 102 ms
 *   against 202 ms (default tables), 100 ms against 247 ms (optimised tables): profiles/mixed_coder_rocprofv3.txt:54-58.
 * hvc_last_mixed_coder_files: how many files of the last hvc_jpeg_encode_batch_mixed_gpu call the GPU coder finished and how
 *   many went to the host coder (either pointer may be NULL). */
HVC_API int hvc_huffman_encode_frames_mixed(hvc_ctx *ctx, const hvc_jpeg_info *infos, const int16_t *coefs,
                                            const size_t *coef_offsets, int n_frames, int tables, uint8_t *out, size_t out_cap,
                                            uint64_t *offsets, int *status, hvc_huff_spec *specs, int where);
HVC_API int hvc_jpeg_encode_batch_mixed_gpu(hvc_ctx *ctx, const uint8_t *const *frames, const hvc_jpeg_info *infos, int *status,
                                            int n_frames, int threads, size_t chunk_bytes, uint8_t *const *jpegs,
                                            const size_t *caps, size_t *sizes, hvc_batch_stats *stats);
HVC_API int hvc_last_mixed_coder_files(const hvc_ctx *ctx, uint64_t *gpu_files, uint64_t *host_files);

/* ------------------------------------------------------------------------- */
/* Mixed batches, ENCODING, from RGB images: what hvc_jpeg_decode_batch_mixed_rgb / _scaled_rgb hand back -- a directory of
 * photographs, or their thumbnails, as RGB images of any size -- made into files again in one call.  One colour pass over
 * images of ANY size and sampling (k_rgb_to_ycc_mixed, csrc/hvc_mixed_rgb.hip: k_ycc_to_rgb_mixed's work decomposition, one
 * wavefront per 64 lanes of one image, and k_rgb_to_ycc's arithmetic per lane) stands in front of the mixed block stage, so
 * every plane byte is what hvc_rgb_to_yuv gives for that image alone and every file byte for byte what hvc_jpeg_encode_rgb
 * gives for it.  Image f is infos[f].width x .height at the sampling infos[f].comp[] names (4:2:0, 4:2:2, 4:4:4; the encoder's
 * rule holds per frame: an even width under 4:2:0 / 4:2:2, an even height under 4:2:0); it is read from rgb + rgb_offsets[f]
 * (or frames[f]) with rows rgb_row_strides[f] bytes apart (>= 3 * width interleaved, >= width planar; an entry of 0, or
 * rgb_row_strides == NULL: tight rows) and planar planes rgb_row_strides[f] * height apart.  One call has one `layout`.
 * Images and planes whose address and strides are multiples of 8 (chroma of 4:2:0 / 4:2:2: of 4) move in 8-byte (4-byte)
 * pieces, the others byte by byte.  With HVC_ARITH_HARDCAML as the ENCODE arithmetic the encoding calls return
 * HVC_E_INVALID_ARG, outputs untouched.  Not here: monochrome.  hvc_jpeg_encode_rgb itself is unchanged.
 *
 * hvc_jpeg_encoder_mixed_rgb_layout (host only, no ctx): per frame what hvc_jpeg_encode_rgb would answer for that geometry --
 *   hvc_jpeg_encoder_layout's code, then hvc_jpeg_encoder_check's, then the even-size rule (HVC_E_INVALID_ARG) -> infos[f],
 *   status[f]; a refused frame takes no room and stops nobody.  A good frame's image lies at rgb_offsets[f], rows
 *   rgb_row_strides[f] = 3 * width (planar: width) rounded up to row_align, records in frame order, each start rounded up to
 *   align (powers of two >= 1, else HVC_E_INVALID_ARG; align 0 = 256, row_align 0 = 1: tight rows); *rgb_total bytes hold all of
 *   them.  pixel_offsets / coef_offsets / *pixel_total / *coef_total are what hvc_jpeg_encoder_mixed_layout gives (align 0: pixel
 *   records on 64 bytes) for the good frames.
 * hvc_rgb_to_yuv_mixed: the way back of hvc_yuv_to_rgb_mixed, argument for argument: frame f's planes are WRITTEN at yuv +
 *   yuv_offsets[f], laid out by infos[f].layout (plane_offset, stride; a component that names its blocks must hold the
 *   samples), from the image at rgb + rgb_offsets[f].  Only each frame's own samples are written: the padding of its planes
 *   stays the caller's.  HVC_MEM_DEVICE: one launch, enqueued on ctx's stream, returns at once, honours hvc_set_profiling (the
 *   pair brackets k_rgb_to_ycc_mixed); HVC_MEM_HOST: staged through context scratch, the call blocks.  For the whole call,
 *   nothing written: HVC_E_INVALID_ARG for an odd size under its sampling, a sampling that is none of the three, a stride below
 *   its row, a negative size; HVC_E_TOO_LARGE: a side above 2^24 or more lanes than the launch can index.  A frame with
 *   width * height == 0 is skipped.
 * hvc_encode_frames_mixed_rgb: RGB images to coefficient records, as hvc_encode_frames_mixed of the planes hvc_rgb_to_yuv makes
 *   of each image in a zeroed padded record.  The padded planes live in context scratch (tight records on 64 bytes, zero-filled
 *   as Plane.create) and never leave the GPU; coefs / coef_offsets / alignment rules and HVC_E_RANGE as hvc_encode_frames_mixed.
 *   A set that is refused leaves nothing behind: both plans are built before anything is enqueued.  HVC_MEM_DEVICE: enqueued on
 *   ctx's stream, honours hvc_set_profiling (the pair brackets k_encode_mixed); HVC_MEM_HOST: the call blocks, and only the
 *   coefficient planes are copied back.
 * hvc_jpeg_encode_batch_mixed_rgb / hvc_jpeg_encode_batch_mixed_rgb_gpu: hvc_jpeg_encode_batch_mixed / _gpu with RGB images as
 *   frames[f]: the same pipelines, chunks (cut by the bytes of the padded pixel records, so the same infos give the same
 *   chunks), statuses, caps / sizes rules, HVC_E_RANGE, stats and hvc_last_mixed_coder_files.  The padding workers copy each
 *   image's rows tight into the pinned ring, the copy stream uploads them into a device RGB slot, and on the compute stream a
 *   memset of the chunk's plane slot and k_rgb_to_ycc_mixed run in front of k_encode_mixed (kernel_ms_sum includes both).  An
 *   image with an odd size under its sampling, or a row stride below its row, gets HVC_E_INVALID_ARG as its own status; a frame
 *   refused before the call keeps its status, jpegs[f] and sizes[f].  Both honour hvc_set_huffman_tables,
 *   hvc_set_restart_interval and hvc_set_host_cpus; under a restart interval the GPU variant hands every file to the host coder. */
HVC_API int hvc_jpeg_encoder_mixed_rgb_layout(const int *widths, const int *heights, const int *chromas, const int *qualities,
                                              int n_frames, int layout, size_t align, size_t row_align, hvc_jpeg_info *infos,
                                              int *status, size_t *rgb_offsets, size_t *rgb_row_strides, size_t *rgb_total,
                                              size_t *pixel_offsets, size_t *coef_offsets, size_t *pixel_total,
                                              size_t *coef_total);
HVC_API int hvc_rgb_to_yuv_mixed(hvc_ctx *ctx, uint8_t *yuv, const size_t *yuv_offsets, const hvc_jpeg_info *infos, int n_frames,
                                 const uint8_t *rgb, const size_t *rgb_offsets, const size_t *rgb_row_strides, int layout,
                                 int where);
HVC_API int hvc_encode_frames_mixed_rgb(hvc_ctx *ctx, const uint8_t *rgb, const size_t *rgb_offsets,
                                        const size_t *rgb_row_strides, int layout, const hvc_jpeg_info *infos, int n_frames,
                                        int16_t *coefs, const size_t *coef_offsets, int where);
HVC_API int hvc_jpeg_encode_batch_mixed_rgb(hvc_ctx *ctx, const uint8_t *const *frames, const size_t *rgb_row_strides, int layout,
                                            const hvc_jpeg_info *infos, int *status, int n_frames, int threads,
                                            size_t chunk_bytes, uint8_t *const *jpegs, const size_t *caps, size_t *sizes,
                                            hvc_batch_stats *stats);
HVC_API int hvc_jpeg_encode_batch_mixed_rgb_gpu(hvc_ctx *ctx, const uint8_t *const *frames, const size_t *rgb_row_strides,
                                                int layout, const hvc_jpeg_info *infos, int *status, int n_frames, int threads,
                                                size_t chunk_bytes, uint8_t *const *jpegs, const size_t *caps, size_t *sizes,
                                                hvc_batch_stats *stats);

/* ------------------------------------------------------------------------- */
/* Resizing: the step that takes the images of a mixed batch -- each of its own size -- to the size the caller names, usually one
 * W x H for all, written as a uniform [n, H, W, 3] or [n, 3, H, W] tensor.  An extension with a named definition (the
 * reference has no resampler): Pillow's Image.resize on 8-bit images, bit for bit, for the filters below; in numpy:
 * tools/resize_reference.py.  Hamming and Lanczos are left out on purpose: they need cos / sin, whose last bit differs
 * between C libraries, so their tables could not be held equal across numpy, the host C++ and Pillow.
 *
 * Filters f with support s:
 *   box       s = 0.5   1 for -0.5 < x <= 0.5, else 0
 *   bilinear  s = 1     1 - |x| for |x| < 1, else 0
 *   bicubic   s = 2     a = -0.5: ((a + 2) |x| - (a + 3)) x^2 + 1 for |x| < 1, (((|x| - 5) |x| + 8) |x| - 4) a for |x| < 2, else 0
 * The coefficients of one axis n_in -> n_out, in IEEE double, one rounding per operation, in exactly this order:
 *   scale = n_in / n_out, fs = max(scale, 1.0), support = s * fs, ss = 1.0 / fs; for each output position xx:
 *   center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), n_in),
 *   count = xmax - xmin, w[i] = f((i + xmin - center + 0.5) * ss) for i < count, ww = the sum of w in index order, w[i] /= ww if
 *   ww != 0, and the integer tap k[i] = (int)(w[i] * 4194304 + 0.5) for w[i] >= 0, (int)(w[i] * 4194304 - 0.5) otherwise ((int)
 *   truncates towards zero; 22 bits).
 * A pass computes, per output sample and channel, clip_0_255((2097152 + SUM k[i] * in[xmin + i]) >> 22) with an arithmetic
 * shift and writes 8-bit samples.  The horizontal pass runs first, to an 8-bit intermediate of n_out_w x h_in; the vertical
 * pass runs over that.  An axis with n_out == n_in is skipped (both: the image is copied).
 *
 * Bounds: a side of at most 2^24; at most HVC_RESIZE_MAX_TAPS = 2048 taps per output position of an axis (an 8192 -> 1 bicubic
 * axis would have 8192); the tables of one call (one per distinct (n_in, n_out, filter): max count * n_out words each) at most
 * 2^24 words together; every output position must satisfy 255 * SUM |k| + 2^21 < 2^31 and |k| < 2^23 (the kernels' int32
 * accumulator and 24-bit multiply -- over sizes 1 .. 8192 to 1 .. 1000 the largest SUM |k| is 1.269 * 2^22, bicubic 69 -> 64,
 * but the plan checks rather than trusts that); out_w * h * out_w < 2^32.  Beyond any of them: HVC_E_TOO_LARGE.
 *
 * hvc_rgb_resize_mixed: image i is widths[i] x heights[i] at src + src_offsets[i], rows src_row_strides[i] apart, and goes to
 *   out_widths[i] x out_heights[i] at dst + dst_offsets[i], rows dst_row_strides[i] apart (a stride array of NULL, or an entry
 *   of 0: tight rows; planar planes lie row stride * height apart, on both sides).  One `layout` (hvc_rgb_layout) and one
 *   `filter` per call; src and dst both live where `where` says.  A uniform tensor is the case of equal output sizes and
 *   dst_offsets[i] = i * frame_stride.  Under k_ycc_to_rgb_mixed's decomposition (csrc/hvc_resize.hip): one launch of
 *   k_resize_h_mixed and one of k_resize_v_mixed per call, a pass no image needs launches nothing; the intermediate lives in
 *   context scratch.  HVC_MEM_DEVICE: enqueued on ctx's stream, returns at once, honours hvc_set_profiling (the pair brackets
 *   both passes); HVC_MEM_HOST: staged through context scratch, the call blocks, only the rows written are downloaded.  Bytes
 *   between rows and between records are never written.  Does not depend on hvc_set_arithmetic.  HVC_E_INVALID_ARG: a size
 *   below 1, a stride below the row, an unknown filter or layout; HVC_E_TOO_LARGE: the bounds above; either way for the whole
 *   call, output untouched.
 * hvc_jpeg_decode_batch_mixed_resized: hvc_jpeg_decode_batch_mixed_scaled_rgb's pipeline (any scale_denom, both readers, chunks,
 *   per-file statuses, HVC_E_RANGE and restart markers as there) ending in the two passes: per chunk the block stage, then
 *   k_ycc_to_rgb_mixed into a device RGB ring slot, then the passes into the output, so the images at decoded size never leave
 *   the GPU.  infos / status: as hvc_jpeg_mixed_layout or any of its kin made them (full-size infos).  File f's image --
 *   its decoded size at 1 / scale_denom -- goes to out_widths[f] x out_heights[f] at dst + dst_offsets[f], rows
 *   dst_row_strides[f] apart (NULL or 0: tight).  A file whose resize is beyond the bounds gets HVC_E_TOO_LARGE (a size below 1
 *   or a stride below the row: HVC_E_INVALID_ARG) as ITS status, and stops nobody; a file that fails leaves its record in dst
 *   untouched.  dst_cap: every good file's record must lie inside (HVC_E_INVALID_ARG).  An unknown filter or layout, and
 *   HVC_ARITH_HARDCAML / _LIBJPEG as the arithmetic (hvc_set_arithmetic): HVC_E_INVALID_ARG for the call, output untouched.
 *   Under hvc_set_mixed_arithmetic(ctx, HVC_ARITH_LIBJPEG) and scale_denom 1 the decode is libjpeg's and a record is Pillow's
 *   Image.open(f).convert("RGB").resize((W, H), filter) byte for byte; scale_denom > 1 is then HVC_E_INVALID_ARG, output untouched.
 *
 * The option block (hvc_resize_opts, the _opts forms of the two calls): what takes the batch to the tensor a model reads.  Every
 * piece has a definition of its own; a NULL or all-zero block is, byte for byte, the call without it.  In numpy:
 * tools/resize_reference.py coefficients_box / resize_box / apply_lut.
 *
 * Box.  Per image box = (x0, y0, x1, y1), four IEEE SINGLE values in the coordinates of the image being resized (file pipeline:
 *   the decoded image at 1 / scale_denom): Pillow's Image.resize(size, resample, box=box), fractional values allowed.  One axis
 *   of n_in samples with the window [in0, in1) to n_out is computed as above except for these two lines:
 *     scale  = (double)(float)(in1 - in0) / n_out      -- the span is subtracted in SINGLE precision, then widened
 *     center = (double)in0 + (xx + 0.5) * scale
 *   fs, support, ss, xmin (clamped at 0), xmax (clamped at n_in), the weights, their normalisation and the 22-bit taps are
 *   unchanged.  Taps may reach outside the box but never outside the image: that is Pillow's behaviour, and why an integer box is
 *   NOT crop().resize().  (With the span taken in double a few results in a thousand differ from Pillow's by one.)
 *   An axis is skipped iff n_out == n_in && in0 == 0 && in1 == n_in.  When both axes run, the horizontal pass covers only the
 *   source rows the vertical pass reads, [ymin[0], ymin[H - 1] + count[H - 1]), and the vertical records are shifted by ymin[0]
 *   (Pillow does the same): the result is identical, the intermediate and the work shrink.
 *   Refused with HVC_E_INVALID_ARG (hvc_rgb_resize_mixed_opts: for the call, output untouched; the file call: as that file's own
 *   status, stopping nobody): a non-finite value; x0 < 0, y0 < 0, x1 > w or y1 > h; a span (float)(in1 - in0) <= 0 (Pillow lets a
 *   zero span through; this library does not).
 * Mirror.  Per image a flag (any non-zero byte).  The output is the unmirrored result with every row reversed left to right
 *   (.transpose(FLIP_LEFT_RIGHT) after the resize).  A mirror makes the horizontal axis run even where it would be skipped, with
 *   the identity table; the host plan emits that axis' records in reverse output order, and no kernel knows about it.
 * Typed output.  out_elem = 0: 8-bit samples, as without the block.  out_elem = 2 or 4: bytes per output element, and `lut` is
 *   HOST memory of 3 * 256 elements of out_elem bytes, indexed [channel][sample]: sample v of channel c is written as lut[c][v]
 *   -- raw bits; the kernel (k_resize_v_mixed_lut, csrc/hvc_resize.hip) does not know what they mean, so the output is exact by
 *   construction for any element type and any formula.  Every image then ends in the vertical pass (the identity table where
 *   that axis is skipped).  Strides, offsets and dst_cap stay in BYTES: a row is out_w * 3 * out_elem bytes interleaved and
 *   out_w * out_elem bytes planar; bytes between rows and records are never written.  out_elem outside {0, 2, 4}, or out_elem
 *   != 0 with lut == NULL: HVC_E_INVALID_ARG for the call, output untouched.
 *   hvc_normalize_lut(mean, std, elem, lut) is the library's own table maker (host only, no context; csrc/hvc_normalize_lut.cpp,
 *   a plain C++ translation unit compiled with -ffp-contract=off): for c < 3, v < 256, in IEEE single with one rounding per
 *   operation, lut[c][v] = ((float)v / 255.0f - mean[c]) / std[c], and for HVC_ELEM_F16 / HVC_ELEM_BF16 one round-to-nearest-
 *   even conversion of that -- torchvision's ToTensor() followed by Normalize(mean, std) on the CPU, bit for bit.  mean, std: 3
 *   values each; lut: 3 * 256 elements of 4 (HVC_ELEM_F32) or 2 bytes.  std[c] == 0, a non-finite mean or std, an unknown elem or
 *   a NULL argument: HVC_E_INVALID_ARG.
 * Bounds under a box: the table key grows to (n_in, n_out, filter, bits of in0, bits of in1, mirrored), so with a box of its own
 *   every image has tables of its own, and a large direct hvc_rgb_resize_mixed_opts call can meet the 2^24 table words
 *   (HVC_E_TOO_LARGE) where the call without boxes would not; the bound is not raised.  The file pipeline plans per chunk and
 *   does not meet it.  The taps and accumulator bounds hold per position as before; out_w * rows * out_w < 2^32 counts the rows
 *   of the horizontal pass's window.
 * hvc_jpeg_decode_batch_mixed_resized_opts keeps the whole matrix of hvc_jpeg_decode_batch_mixed_resized (chunks, per-file
 *   statuses, both readers, restart markers, any scale_denom, hvc_set_mixed_arithmetic(ctx, HVC_ARITH_LIBJPEG) at scale 1, under
 *   which an 8-bit record is Image.open(f).convert("RGB").resize((W, H), filter, box=box) byte for byte).  The block stage and
 *   the colour pass still produce the WHOLE image at decoded size; stages that decode and convert only the box are a later step. */
typedef enum { HVC_RESIZE_BOX = 0, HVC_RESIZE_BILINEAR = 1, HVC_RESIZE_BICUBIC = 2 } hvc_resize_filter;
typedef enum { HVC_ELEM_F32 = 1, HVC_ELEM_F16 = 2, HVC_ELEM_BF16 = 3 } hvc_elem; /* hvc_normalize_lut's element types */
typedef struct hvc_resize_opts {
    const float *boxes;      /* NULL, or 4 per image: x0, y0, x1, y1 */
    const uint8_t *mirror;   /* NULL, or 1 per image */
    int out_elem;            /* 0, 2, 4: bytes per output element */
    const void *lut;         /* host, 3 * 256 elements of out_elem bytes, when out_elem != 0 */
} hvc_resize_opts;
#define HVC_RESIZE_MAX_TAPS 2048
HVC_API int hvc_rgb_resize_mixed(hvc_ctx *ctx, const uint8_t *src, const size_t *src_offsets, const size_t *src_row_strides,
                                 const int *widths, const int *heights, int n_images, uint8_t *dst, const size_t *dst_offsets,
                                 const size_t *dst_row_strides, const int *out_widths, const int *out_heights, int layout,
                                 int filter, int where);
HVC_API int hvc_jpeg_decode_batch_mixed_resized(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_files,
                                                int threads, size_t chunk_bytes, int scale_denom, const hvc_jpeg_info *infos,
                                                int *status, const int *out_widths, const int *out_heights,
                                                const size_t *dst_offsets, const size_t *dst_row_strides, uint8_t *dst,
                                                size_t dst_cap, int layout, int filter, int where, hvc_batch_stats *stats);
HVC_API int hvc_rgb_resize_mixed_opts(hvc_ctx *ctx, const uint8_t *src, const size_t *src_offsets, const size_t *src_row_strides,
                                      const int *widths, const int *heights, int n_images, uint8_t *dst, const size_t *dst_offsets,
                                      const size_t *dst_row_strides, const int *out_widths, const int *out_heights, int layout,
                                      int filter, int where, const hvc_resize_opts *opts);
HVC_API int hvc_jpeg_decode_batch_mixed_resized_opts(hvc_ctx *ctx, const uint8_t *const *jpegs, const size_t *sizes, int n_files,
                                                     int threads, size_t chunk_bytes, int scale_denom, const hvc_jpeg_info *infos,
                                                     int *status, const int *out_widths, const int *out_heights,
                                                     const size_t *dst_offsets, const size_t *dst_row_strides, uint8_t *dst,
                                                     size_t dst_cap, int layout, int filter, int where, hvc_batch_stats *stats,
                                                     const hvc_resize_opts *opts);
HVC_API int hvc_normalize_lut(const float *mean, const float *std, int elem, void *lut);

/* K5 (no counterpart in the reference): what a benchmark or a pipeline produced, said in
 * 64 bits per record without bringing the records back.  For r < n_records
 *     sums[r] = SUM_i (byte_i + 1) * ((2 i + 1) * 0x9E3779B97F4A7C15)   mod 2^64,  i = byte index in record r
 * over data + r * record_stride, record_bytes bytes each.  data lives where `where` says (host data is uploaded
 * first); sums is host memory; the call returns when sums is complete.  The same 64 bits follow from three
 * lines of numpy on any machine (tests/helpers.py checksum_records), which is how the CPU suite pins the
 * benchmarks' outputs to the model. */
HVC_API int hvc_checksum_records(hvc_ctx *ctx, const void *data, size_t record_bytes, size_t record_stride,
                                 int n_records, uint64_t *sums, int where);

/* ------------------------------------------------------------------------- */
/* The asynchronous seam ("async batch API: submit(frame batch, stream slot) / wait(slot)"; BASELINE.json
 * north_star: "host-side Huffman decode feeds pinned coefficient buffers via hipMemcpyAsync on a side stream overlapped
 * with the IDCT kernel").  For the caller that keeps the reference's OWN sequential Huffman reader
 * (decoder.ml:118-140, untouched) and wants what hvc_jpeg_decode_batch gives the library's reader: while the GPU works
 * on batch k, the caller's reader fills batch k + 1.
 *
 * A context has HVC_SLOTS slots; a slot carries one batch in flight:
 *     submit:  host coefficient records --hipMemcpyAsync, copy stream--> device --block stage, ctx's stream--> device pixels
 *              --hipMemcpyAsync, download stream--> host pixel records          (decode; the encoder mirror runs the other way)
 * and returns at once.  Three streams, so slot k + 1's upload, slot k's kernel and slot k - 1's download overlap, and the
 * link carries both directions.  hvc_wait(ctx, slot) blocks until the slot's results are visible and frees the slot.
 * The host buffers of a submission must stay valid and unmodified (coefficients) / unread (pixels) until its hvc_wait
 * (or hvc_destroy): the copy engines read and write them on their own time, and memory freed under them is a GPU page
 * fault, not a status code.
 * They should be PINNED -- from hvc_host_alloc, or the caller's own page-aligned memory passed once through
 * hvc_host_register: from pageable memory hipMemcpyAsync stages through the runtime's bounce buffers and holds its
 * caller (the result is the same, the overlap is gone).
 * Like everything on a context the slot calls are not thread-safe among themselves; what the caller does meanwhile on
 * its own memory (filling the next slot's buffer, on any number of threads) is its business.
 * Errors: HVC_E_BUSY = the slot still holds a submission (hvc_wait first); everything hvc_decode_frames /
 * hvc_encode_frames answer to the same arguments; a HIP failure inside the slot's work is reported by ITS hvc_wait.
 * Measured on MI355X: 1080p 4:2:0 records from pinned slots of 64 frames, the caller's threads refilling
 * the next slot meanwhile: 18.4 - 18.7 Gpixel/s at 56 - 57 GB/s of upload (the link's rate), 17 Gpixel/s with the pixel
 * records coming back as well; the blocking HVC_MEM_HOST call on pageable memory: 15.8. */
enum { HVC_SLOTS = 4 };

/* Pinned host memory (hipHostMalloc): 4 KiB-aligned, usable as a Bigarray (Ctypes.bigarray_of_ptr) or any byte buffer. */
HVC_API int hvc_host_alloc(hvc_ctx *ctx, size_t bytes, void **out);
HVC_API int hvc_host_free(hvc_ctx *ctx, void *p);
/* Pins memory the caller already owns (hipHostRegister): [p, p + bytes) stays where it is and becomes a DMA source /
 * target; hvc_host_unregister before freeing it.  WHOLE PAGES ONLY -- p and bytes multiples of the page size
 * (posix_memalign / mmap / aligned_alloc; HVC_E_ALIGNMENT otherwise), pages that hold nothing but this buffer: the HIP
 * runtime finds registered memory by page, and a pageable buffer that shares a registered range's last page is copied
 * through that range's mapping until the GPU faults where it ends.  (A Bigarray.Array1 lives outside the OCaml heap and
 * never moves, but Bigarray.create's memory is malloc's: take hvc_host_alloc for those, as the patch's Hvc.pinned_* do.) */
HVC_API int hvc_host_register(hvc_ctx *ctx, void *p, size_t bytes);
HVC_API int hvc_host_unregister(hvc_ctx *ctx, void *p);

/* hvc_decode_frames (same arguments, same arithmetic: decoder.ml:142-149, 213-224; dct.ml:11-107) on host coefficient
 * records, asynchronously in `slot`.  pixels_where = HVC_MEM_HOST: the pixel records are downloaded into `pixels`
 * (only the bytes the kernels wrote: the component planes); HVC_MEM_DEVICE: `pixels` is device memory of ctx's GPU
 * and the block stage writes it directly (hvc_wait then says the kernel is done). */
HVC_API int hvc_decode_frames_submit(hvc_ctx *ctx, int slot, const int16_t *coefs, size_t coef_frame_stride,
                                     const uint16_t *qtabs, int n_qtabs, const hvc_component *comps, int n_comp,
                                     int n_frames, uint8_t *pixels, size_t pixel_frame_stride, int pixels_where);
/* The encoder mirror: hvc_encode_frames (encoder.ml:81-108; dct.ml:109-196) on host pixel records; the coefficient
 * records go to `coefs`, host (downloaded: the coefficient planes) or device as coefs_where says. */
HVC_API int hvc_encode_frames_submit(hvc_ctx *ctx, int slot, const uint8_t *pixels, size_t pixel_frame_stride,
                                     const uint16_t *qtabs, int n_qtabs, const hvc_component *comps, int n_comp,
                                     int n_frames, int16_t *coefs, size_t coef_frame_stride, int coefs_where);
/* Blocks until the slot's submission is complete (an idle slot: returns at once); the slot is free afterwards.
 * hvc_slot_query: the same question without waiting (*done = 1: hvc_wait will not block). */
HVC_API int hvc_wait(hvc_ctx *ctx, int slot);
HVC_API int hvc_slot_query(hvc_ctx *ctx, int slot, int *done);
/* What the slot's LAST completed submission cost, from HIP events on the three streams (valid after its hvc_wait):
 * upload, block stage (incl. the fix-up kernels), download; 0 for a stage it did not have. */
typedef struct hvc_slot_stats {
    double h2d_ms, kernel_ms, d2h_ms;
    uint64_t h2d_bytes, d2h_bytes;
} hvc_slot_stats;
HVC_API int hvc_slot_last_stats(hvc_ctx *ctx, int slot, hvc_slot_stats *stats);

/* Fixed-point DCT: the model's parametric Dct.Fixed_point (jpeg/model/src/dct.ml:443-482) and the precision search of
 * jpeg/bin/dct.ml, bit for bit.  The ROM of rom_prec p is round_nearest(M * 2^p), M the static x86 forward matrix
 * (dct.ml:255-337); the inverse uses its transpose.  T = round(C X, p - tp), Y = round(T C^T, p + tp), rounding ties away
 * from zero (a negative shift is a left shift).  Accepted: 0 <= rom_prec <= 16, 0 <= transpose_prec <= 8, |x| <= 2048
 * into the forward transform and |x| <= 32768 (the largest |Y| of any accepted forward call) into the inverse; anything
 * else is HVC_E_RANGE, never a wrong result.  The float64 reference is fmul (fmul F X) F^T (dct.ml:210-218), F = M or M^T,
 * each sum from 0.0 in order k = 0..7, no fused multiply-add.  Blocks are 64 int32 in row-major order.
 *
 * hvc_dct_blocks is the search's input generator, a pure function of (seed, range, block index): element j of block i
 * is ((w * 2 range) >> 32) - range in [-range, range), w the low (j even) or high (j odd) 32 bits of the (32 i + j / 2)-th
 * output of SplitMix64 seeded with `seed`.  Upstream draws from OCaml's Random instead; this generator makes every
 * configuration of a search see the same blocks and any worst block reproducible from its index.  1 <= range <= 32768.
 *
 * hvc_dct_error_search runs blocks first_block .. first_block + n_blocks - 1 through every configuration.  FORWARD and
 * INVERSE use the fwd_* / inv_* fields and the error of a block is max |fixed - reference| over its 64 outputs; ROUND_TRIP
 * uses both and the error is max |x - inverse(forward(x))| (an integer).  range <= 2048 (forward, round trip) or
 * <= 32768 (inverse).  results[i] is the largest error and the smallest block index that has it, the same for any split
 * of the block range.  All parameters are checked before anything runs: HVC_E_RANGE and HVC_E_INVALID_ARG write nothing.
 * cfg and results are host memory; the call blocks.
 *
 * hvc_dct_fixed / hvc_dct_reference: explicit blocks, `where` as elsewhere (device memory: in and out 4-byte aligned,
 * 8-byte for doubles).  hvc_dct_fixed always waits for its range check: under HVC_MEM_DEVICE a block with an input out of
 * range is left unwritten and the call returns HVC_E_RANGE. */
#define HVC_DCT_FORWARD 0
#define HVC_DCT_INVERSE 1
#define HVC_DCT_ROUND_TRIP 2
typedef struct hvc_dct_config {
    int mode, fwd_rom_prec, fwd_transpose_prec, inv_rom_prec, inv_transpose_prec;
} hvc_dct_config;
typedef struct hvc_dct_error {
    double max_error;
    uint64_t worst_block;
} hvc_dct_error;
HVC_API int hvc_dct_rom(int rom_prec, int32_t *rom64);   /* host only: the forward ROM the kernels use */
HVC_API int hvc_dct_matrix(double *m64);                 /* host only: the float64 matrix M */
HVC_API int hvc_dct_blocks(uint64_t seed, int range, uint64_t first, size_t n, int32_t *out); /* host only */
HVC_API int hvc_dct_fixed(hvc_ctx *ctx, int direction, int rom_prec, int transpose_prec, const int32_t *in, int32_t *out,
                          size_t n_blocks, int where);
HVC_API int hvc_dct_reference(hvc_ctx *ctx, int direction, const int32_t *in, double *out, size_t n_blocks, int where);
HVC_API int hvc_dct_error_search(hvc_ctx *ctx, const hvc_dct_config *cfg, size_t n_cfg, uint64_t seed, int range,
                                 uint64_t first_block, uint64_t n_blocks, hvc_dct_error *results);

/* Device memory helpers so that a binding needs no HIP of its own. */
HVC_API int hvc_device_alloc(hvc_ctx *ctx, size_t bytes, void **out);
HVC_API int hvc_device_free(hvc_ctx *ctx, void *p);
HVC_API int hvc_memcpy_h2d(hvc_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
HVC_API int hvc_memcpy_d2h(hvc_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* HVC_JPEG_H */
