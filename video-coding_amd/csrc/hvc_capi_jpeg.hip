// hvc_capi_jpeg.hip -- files through the C ABI.  One at a time: hvc_jpeg_decode, hvc_jpeg_decode_yuv444 and hvc_jpeg_decode_rgb
// (one skeleton, decode_one_file, with a sink each), hvc_jpeg_decode_scaled and hvc_jpeg_decode_scaled_rgb (host reader only),
// hvc_jpeg_encode, hvc_jpeg_encode_rgb.  Batches: BASELINE's configuration 3, the pipeline with the Huffman reader on the host
// (decode_batch_impl behind hvc_jpeg_decode_batch, _batch_yuv444 and _batch_scaled), and hvc_jpeg_decode_batch_rgb over either
// pipeline.
#include "hvc_batch.h"
#include "hvc_mixed_plan.h"
#include "hvc_mixed_rgb_plan.h"

// ---------------------------------------------------------------------------
// single-frame conveniences (host memory)

// One file: Huffman reader on the GPU (hvc_hdec.hip) into device scratch; *used = 0 when the stream needs the
// host decoder (nothing usable on the device then).
static int single_frame_coefs_on_device(hvc_ctx *c, const uint8_t *jpeg, size_t n, const hvc_jpeg_info *info, int *used,
                                        AfterReader *after) {
    *used = 0;
    // Below ~128 kB the host reader is done before the GPU decoder's launches and synchronisations are
    // (single calls on 1080p files: 64 kB file 0.39 ms on the host vs 0.8 ms; 228 kB 1.7 vs 0.8 ms; 967 kB 3.9 vs 1.6 ms).
    if (n < 128u * 1024u) return HVC_OK;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    int r = grow(c, c->gd_coefs, info->coef_count * sizeof(int16_t));
    if (r) return r;
    if (c->decode_kernel != 1 && c->decode_kernel != 3) { // (the A/B alternates read the DC from the record)
        const size_t blocks = info->coef_count / 64;
        if ((r = grow(c, c->gd_dcv, ((blocks + 127) & ~(size_t)127) * sizeof(int16_t)))) return r;
        after->dc_plane = c->gd_dcv.as<int16_t>();
        after->dc_fs = blocks;
    }
    return gpu_entropy_decode(c, &jpeg, &n, 1, *info, c->gd_coefs.as<int16_t>(), info->coef_count, used, after);
}

// One file whose header is read and whose arguments are checked, to the caller's memory.  What the entry points differ in
// is their sink:
//   enqueue(d_coefs, o)  enqueues on c->stream the block stage of the device record d_coefs with the options o and
//                        everything that brings its result to the caller's memory; it does not synchronise
//   host(coefs)          decodes a host record straight to the caller's memory -- or nullptr: host records are uploaded
// A file of 128 kB and more goes to the GPU reader with enqueue() behind it before the reader's verdict is known
// (AfterReader); what the reader cannot take, the host reader reads, and blocks whose DC leaves int16 go through the int64
// fix-up with their true DCs -- the model's output for such a stream (decoder.ml:143).
template <class Enqueue, class Host>
static int decode_one_file(hvc_ctx *c, const uint8_t *jpeg, size_t n, const hvc_jpeg_info *info, Enqueue enqueue, Host host) {
    int on_gpu = 0;
    AfterReader after;
    auto from_reader = [&]() -> int { // the record the reader leaves at c->gd_coefs
        DeviceGuard g(c->device);
        DecodeOpts o(c); // (profiling as the context has it)
        o.dc_plane = after.dc_plane;
        o.dc_fs = after.dc_fs;
        return enqueue(c->gd_coefs.as<const int16_t>(), o);
    };
    after.enqueue = from_reader;
    int r = single_frame_coefs_on_device(c, jpeg, n, info, &on_gpu, &after);
    if (r) return r;
    if (on_gpu) {
        if (after.speculated) return HVC_OK; // (the reader's one synchronisation covered the download)
        DeviceGuard g(c->device);
        if ((r = from_reader())) return r; // (what was enqueued ran on records the reader had not finished)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return HVC_OK;
    }
    std::vector<int16_t> coefs;
    std::vector<hvc::WideDc> wide;
    std::vector<WideFix> fix;
    try {
        coefs.resize(info->coef_count);
    } catch (const std::bad_alloc &) {
        return HVC_E_OUT_OF_MEMORY;
    }
    if ((r = hvc::entropy_decode_wide(jpeg, n, info, coefs.data(), wide))) return r;
    if constexpr (!std::is_null_pointer<Host>::value)
        if (wide.empty()) return host(coefs.data());
    try {
        for (const hvc::WideDc &w : wide) fix.push_back(WideFix{0, w.block, w.dc});
    } catch (const std::bad_alloc &) {
        return HVC_E_OUT_OF_MEMORY;
    }
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    const size_t cb = info->coef_count * sizeof(int16_t);
    if ((r = grow(c, c->d_in, cb))) return r;
    HIPCHK(c, hipMemcpyAsync(c->d_in.p, coefs.data(), cb, hipMemcpyHostToDevice, c->stream));
    DecodeOpts o(c);
    o.profile = false;
    o.wide = &fix;
    if ((r = enqueue(c->d_in.as<const int16_t>(), o))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HVC_OK;
}

// the sink of hvc_jpeg_decode and hvc_jpeg_decode_yuv444: the block stage's own output, from device records through c->d_out
// (ALL components in one launch, one download), from host records as a host-memory call
static int decode_file_to(hvc_ctx *c, const uint8_t *jpeg, size_t n, const OutputForm &form, uint8_t *dst) {
    return decode_one_file(
        c, jpeg, n, &form.info,
        [&](const int16_t *d_coefs, const DecodeOpts &o) -> int {
            int e = grow(c, c->d_out, form.out_bytes);
            if (e) return e;
            if ((e = form.run(c, d_coefs, 1, c->d_out.as<uint8_t>(), form.out_bytes, HVC_MEM_DEVICE, o))) return e;
            HIPCHK(c, hipMemcpyAsync(dst, c->d_out.p, form.out_bytes, hipMemcpyDeviceToHost, c->stream));
            return HVC_OK;
        },
        [&](const int16_t *coefs) { return form.run(c, coefs, 1, dst, form.out_bytes, HVC_MEM_HOST, DecodeOpts(c)); });
}

// Decoder.decode_a_frame minus the crop (decoder.ml:422-427)
int hvc_jpeg_decode_yuv444(hvc_ctx *c, const uint8_t *jpeg, size_t n, hvc_jpeg_info *info, uint8_t *frame,
                           size_t frame_cap) try {
    if (!c || !jpeg || !info || !frame) return HVC_E_INVALID_ARG;
    if (c->arith != HVC_ARITH_MODEL) return HVC_E_INVALID_ARG; // (no RTL form of the fused path: hvc_set_arithmetic)
    hvc::RestartScope honour(c->honour_restart); // (hvc_set_restart_markers; off = the model's behaviour)
    int r = hvc_jpeg_read_header(jpeg, n, info);
    if (r) return r;
    if (!is_420_scan(*info)) return HVC_E_INVALID_ARG; // (Frame.infer_chroma_subsampling, common/src/frame.ml:42-61)
    OutputForm form(OutputForm::YUV444);
    form.of(*info);
    if (frame_cap < form.out_bytes) return HVC_E_INVALID_ARG;
    if (info->width == 0 || info->height == 0) // a frame without a sample: the model decodes no block (decoder.ml:377-395)
        return hvc_jpeg_entropy_decode(jpeg, n, info, nullptr); // and of_420 of empty planes is an empty frame; the tables are still looked up
    return decode_file_to(c, jpeg, n, form, frame);
} HVC_ABI_CATCH

int hvc_jpeg_decode(hvc_ctx *c, const uint8_t *jpeg, size_t n, hvc_jpeg_info *info, uint8_t *pixels, size_t pixel_cap) try {
    if (!c || !jpeg || !info) return HVC_E_INVALID_ARG;
    hvc::RestartScope honour(c->honour_restart); // (hvc_set_restart_markers; off = the model's behaviour)
    int r = hvc_jpeg_read_header(jpeg, n, info);
    if (r) return r;
    if (pixel_cap < info->pixel_bytes || (!pixels && info->pixel_bytes)) return HVC_E_INVALID_ARG; // (planes without a sample need no memory)
    OutputForm form(OutputForm::PLANES);
    form.of(*info);
    return decode_file_to(c, jpeg, n, form, pixels);
} HVC_ABI_CATCH

// The tail of the single-file RGB calls: the planes `pi` describes (a file's info, or its scaled form) lie in c->d_aux, the
// image is made of them in c->d_aux2 and only its bytes come back.
struct RgbTail {
    int sampling = 0;
    RgbImage im;
    int scratch(hvc_ctx *c, const hvc_jpeg_info &pi) const { // (before anything is written to c->d_aux)
        const int r = grow(c, c->d_aux, pi.pixel_bytes);
        return r ? r : grow(c, c->d_aux2, rgb_bytes(im, 1));
    }
    int enqueue(hvc_ctx *c, const hvc_jpeg_info &pi, uint8_t *rgb) const { // colour pass and download on c->stream
        int cw, ch;
        rgb_chroma_window(sampling, pi.width, pi.height, cw, ch);
        HIPCHK(c, ycc_to_rgb_device(c->d_aux.as<const uint8_t>(), pi.pixel_bytes, pi.layout, sampling, pi.width, pi.height, cw, ch, 1,
                                    c->d_aux2.as<uint8_t>(), im, c->stream, c->arith));
        HIPCHK(c, rgb_download(c->d_aux2.as<const uint8_t>(), rgb, im, 1, c->stream));
        return HVC_OK;
    }
};

// hvc_jpeg_decode with the colour pass behind the block stage: the planes stay in device scratch
int hvc_jpeg_decode_rgb(hvc_ctx *c, const uint8_t *jpeg, size_t n, hvc_jpeg_info *info, uint8_t *rgb, size_t rgb_cap, size_t rgb_row_stride,
                        int layout) try {
    if (!c || !jpeg || !info || !rgb) return HVC_E_INVALID_ARG;
    hvc::RestartScope honour(c->honour_restart); // (hvc_set_restart_markers; off = the model's behaviour)
    int r = hvc_jpeg_read_header(jpeg, n, info);
    if (r) return r;
    RgbTail tail;
    tail.sampling = rgb_sampling_of(*info);
    if (!tail.sampling || !rgb_image(layout, info->width, info->height, rgb_row_stride, 0, tail.im)) return HVC_E_INVALID_ARG;
    if (rgb_cap < rgb_bytes(tail.im, 1)) return HVC_E_INVALID_ARG;
    if (info->width == 0 || info->height == 0 || info->pixel_bytes == 0) // a frame without a sample: the file is still read as the model reads it
        return hvc_jpeg_entropy_decode(jpeg, n, info, nullptr);
    {
        DeviceGuard g(c->device);
        if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
        if ((r = tail.scratch(c, *info))) return r;
    }
    OutputForm form(OutputForm::PLANES);
    form.of(*info);
    return decode_one_file(
        c, jpeg, n, info,
        [&](const int16_t *d_coefs, const DecodeOpts &o) -> int {
            const int e = form.run(c, d_coefs, 1, c->d_aux.as<uint8_t>(), form.out_bytes, HVC_MEM_DEVICE, o);
            return e ? e : tail.enqueue(c, *info, rgb);
        },
        nullptr); // (the host reader's record is uploaded)
} HVC_ABI_CATCH

// ---------------------------------------------------------------------------
// Decoding at reduced size (include/hvc_jpeg.h): the geometry, one file to planes, one file to RGB, a batch

int hvc_jpeg_scaled_info(const hvc_jpeg_info *info, int scale_denom, hvc_jpeg_info *out) try {
    const int N = scaled_side(scale_denom);
    if (!info || !out || !N || info->n_comp < 0 || info->n_comp > 4) return HVC_E_INVALID_ARG;
    scaled_info(*info, N, *out);
    return HVC_OK;
} HVC_ABI_CATCH

// header of one file for the scaled entry points: `form` = its scaled form, *info = the SCALED info, `coefs` sized for its record
static int read_for_scaled(hvc_ctx *c, const uint8_t *jpeg, size_t n, hvc_jpeg_info *info, OutputForm &form, std::vector<int16_t> &coefs) {
    if (!form.known()) return HVC_E_INVALID_ARG;
    if (c->arith != HVC_ARITH_MODEL) return HVC_E_INVALID_ARG; // (no RTL form of the scaled path)
    hvc_jpeg_info full;
    int r = hvc_jpeg_read_header(jpeg, n, &full);
    if (r) return r;
    form.of(full);
    *info = form.sinfo;
    try {
        coefs.resize(full.coef_count);
    } catch (const std::bad_alloc &) {
        return HVC_E_OUT_OF_MEMORY;
    }
    return HVC_OK;
}
// (after the caller's checks of its output's size) the record: HVC_E_RANGE where a block's absolute DC leaves int16
static int entropy_for_scaled(const uint8_t *jpeg, size_t n, const hvc_jpeg_info &full, std::vector<int16_t> &coefs) {
    std::vector<hvc::WideDc> wide;
    const int r = hvc::entropy_decode_wide(jpeg, n, &full, coefs.data(), wide);
    return r ? r : wide.empty() ? HVC_OK : HVC_E_RANGE;
}

int hvc_jpeg_decode_scaled(hvc_ctx *c, const uint8_t *jpeg, size_t n, int scale_denom, hvc_jpeg_info *info, uint8_t *pixels,
                           size_t pixel_cap) try {
    if (!c || !jpeg || !info) return HVC_E_INVALID_ARG;
    if (scale_denom == 1) return hvc_jpeg_decode(c, jpeg, n, info, pixels, pixel_cap); // full size: that call, with all its rules
    hvc::RestartScope honour(c->honour_restart); // (hvc_set_restart_markers; off = the model's behaviour)
    OutputForm form(OutputForm::SCALED, scale_denom);
    std::vector<int16_t> coefs;
    int r = read_for_scaled(c, jpeg, n, info, form, coefs);
    if (r) return r;
    if (pixel_cap < info->pixel_bytes || (!pixels && info->pixel_bytes)) return HVC_E_INVALID_ARG;
    if ((r = entropy_for_scaled(jpeg, n, form.info, coefs))) return r;
    return form.run(c, coefs.data(), 1, pixels, form.out_bytes, HVC_MEM_HOST, DecodeOpts(c));
} HVC_ABI_CATCH

int hvc_jpeg_decode_scaled_rgb(hvc_ctx *c, const uint8_t *jpeg, size_t n, int scale_denom, hvc_jpeg_info *info, uint8_t *rgb,
                               size_t rgb_cap, size_t rgb_row_stride, int layout) try {
    if (!c || !jpeg || !info || !rgb) return HVC_E_INVALID_ARG;
    if (scale_denom == 1) return hvc_jpeg_decode_rgb(c, jpeg, n, info, rgb, rgb_cap, rgb_row_stride, layout); // full size: that call
    hvc::RestartScope honour(c->honour_restart);
    OutputForm form(OutputForm::SCALED, scale_denom);
    std::vector<int16_t> coefs;
    int r = read_for_scaled(c, jpeg, n, info, form, coefs);
    if (r) return r;
    RgbTail tail;
    tail.sampling = rgb_sampling_of(form.info);
    if (!tail.sampling || !rgb_image(layout, info->width, info->height, rgb_row_stride, 0, tail.im)) return HVC_E_INVALID_ARG;
    if (rgb_cap < rgb_bytes(tail.im, 1)) return HVC_E_INVALID_ARG;
    if ((r = entropy_for_scaled(jpeg, n, form.info, coefs))) return r;
    if (info->width == 0 || info->height == 0 || info->pixel_bytes == 0) return HVC_OK; // a frame without a sample
    int cw, ch;
    rgb_chroma_window(tail.sampling, info->width, info->height, cw, ch);
    // the window lies inside the scaled decoded chroma planes: the MCU-rounded size divided by scale_denom is even
    if (tail.sampling != HVC_YUV_400 && (cw > info->comp[1].decoded_width || ch > info->comp[1].decoded_height ||
                                         cw > info->comp[2].decoded_width || ch > info->comp[2].decoded_height))
        return HVC_E_INTERNAL;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    const size_t cb = form.info.coef_count * sizeof(int16_t);
    if ((r = tail.scratch(c, *info))) return r;
    if ((r = grow(c, c->d_in, cb))) return r;
    HIPCHK(c, hipMemcpyAsync(c->d_in.p, coefs.data(), cb, hipMemcpyHostToDevice, c->stream));
    DecodeOpts o(c);
    o.profile = false;
    if ((r = form.run(c, c->d_in.as<const int16_t>(), 1, c->d_aux.as<uint8_t>(), form.out_bytes, HVC_MEM_DEVICE, o))) return r;
    if ((r = tail.enqueue(c, *info, rgb))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HVC_OK;
} HVC_ABI_CATCH

int hvc_jpeg_decode_batch_scaled(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int threads,
                                 int frames_per_chunk, int gpu_reader, int scale_denom, uint8_t *pixels, size_t pixel_fs, int where,
                                 hvc_batch_stats *stats) try {
    if (!c || !scaled_side(scale_denom)) return HVC_E_INVALID_ARG;
    if (scale_denom != 1 && c->arith != HVC_ARITH_MODEL) return HVC_E_INVALID_ARG; // (no RTL form of the scaled path)
    const OutputForm form(OutputForm::SCALED, scale_denom);
    return gpu_reader ? decode_batch_gpu(c, jpegs, sizes, n_frames, threads, frames_per_chunk, pixels, pixel_fs, where, stats, form)
                      : decode_batch_impl(c, jpegs, sizes, n_frames, threads, frames_per_chunk, pixels, pixel_fs, where, stats, form);
} HVC_ABI_CATCH

// Encoder.encode_420/422/444 (encoder.ml:512-541)

// The device half of hvc_jpeg_encode / hvc_jpeg_encode_rgb: scratch for one frame (padded planes c->d_in, records c->d_out,
// segment c->hd_out), and, once the padded planes are at c->d_in, forward block stage, Huffman coder, header + segment + EOI.
static int encode_scratch(hvc_ctx *c, const hvc_jpeg_info &info, size_t *seg_cap) {
    const size_t coef_bytes = info.coef_count * sizeof(int16_t);
    const int ri = c->restart_interval; // DRI + RSTn every ri MCUs (hvc_set_restart_interval)
    const size_t n_ivl = ri ? (info.coef_count / 64 + (size_t)ri - 1) / (size_t)ri : 0; // (at most: an MCU holds >= 3 blocks)
    *seg_cap = (info.coef_count / 64) * 243 + 64 + 4 * n_ivl; // worst case incl. stuffing; a (stuffed) pad byte + marker per interval
    int r;
    if ((r = grow(c, c->d_in, info.pixel_bytes))) return r;
    if ((r = grow(c, c->d_out, coef_bytes))) return r;
    return grow(c, c->hd_out, *seg_cap);
}
static int encode_padded_on_device(hvc_ctx *c, const hvc_jpeg_info &info, size_t seg_cap, uint8_t *out, size_t cap, size_t *out_len);

int hvc_jpeg_encode(hvc_ctx *c, const uint8_t *y, const uint8_t *u, const uint8_t *v, int width, int height, int chroma,
                    int quality, uint8_t *out, size_t cap, size_t *out_len) try {
    if (!c || !y || !u || !v || !out_len) return HVC_E_INVALID_ARG;
    hvc_jpeg_info info;
    int r = hvc_jpeg_encoder_layout(width, height, chroma, quality, &info);
    if (r) return r;
    if ((r = hvc_jpeg_encoder_check(&info))) return r; // the model raises for this geometry
    std::vector<uint8_t> planes;
    try {
        planes.assign(info.pixel_bytes, 0); // Plane.create is zero-filled (plane.ml:11-17)
    } catch (const std::bad_alloc &) {
        return HVC_E_OUT_OF_MEMORY;
    }
    // Plane.blit_available of the frame's planes into the padded ones (encoder.ml:514-516; frame.ml:10-41)
    const uint8_t *src[3] = {y, u, v};
    const int cw = chroma == 444 ? width : width / 2, ch = chroma == 420 ? height / 2 : height;
    const int sw[3] = {width, cw, cw}, sh[3] = {height, ch, ch};
    for (int i = 0; i < 3; i++) {
        if (c->enc_libjpeg && sw[i] > 0 && sh[i] > 0) { // hvc_set_encode_libjpeg: libjpeg repeats the last column and row
            hvc::pad_plane_replicate(src[i], sw[i], sh[i], planes.data() + info.layout[i].plane_offset, info.comp[i].decoded_width,
                                     info.comp[i].decoded_height, info.layout[i].stride);
            continue;
        }
        const int bw = sw[i] < info.comp[i].decoded_width ? sw[i] : info.comp[i].decoded_width;
        const int bh = sh[i] < info.comp[i].decoded_height ? sh[i] : info.comp[i].decoded_height;
        for (int row = 0; row < bh; row++)
            std::memcpy(planes.data() + info.layout[i].plane_offset + (size_t)row * info.layout[i].stride,
                        src[i] + (size_t)row * sw[i], (size_t)bw);
    }
    // forward block stage and Huffman coder both on the device; only the entropy-coded segment comes back
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    size_t seg_cap = 0;
    if ((r = encode_scratch(c, info, &seg_cap))) return r;
    HIPCHK(c, hipMemcpyAsync(c->d_in.p, planes.data(), info.pixel_bytes, hipMemcpyHostToDevice, c->stream));
    return encode_padded_on_device(c, info, seg_cap, out, cap, out_len);
} HVC_ABI_CATCH

static int encode_padded_on_device(hvc_ctx *c, const hvc_jpeg_info &info, size_t seg_cap, uint8_t *out, size_t cap, size_t *out_len) {
    int r;
    std::vector<uint8_t> header;
    const int ri = c->restart_interval;
    EncodeOpts o(c);
    o.profile = false;
    o.edges = &info; // (hvc_set_encode_libjpeg: the file's dummy blocks)
    r = encode_frames_impl(c, c->d_in.as<const uint8_t>(), info.pixel_bytes, &info.qtabs[0][0], info.n_qtabs, info.layout, 3, 1,
                           c->d_out.as<int16_t>(), info.coef_count, HVC_MEM_DEVICE, o);
    if (r) return r;
    hvc::HuffParams P;
    const bool opt = c->huff_tables == HVC_HUFF_OPTIMISED; // the frame's own tables (hvc_set_huffman_tables)
    if ((r = huffman_prepare(c, &info, c->d_out.as<const int16_t>(), info.coef_count, 1, c->hd_out.as<uint8_t>(), seg_cap, nullptr, P,
                             opt, ri)))
        return r;
    HIPCHK(c, hvc::launch_huffman_encode(P, c->stream));
    unsigned status = 0;
    unsigned long long off[2] = {0, 0};
    hvc_huff_spec specs[4];
    HIPCHK(c, hipMemcpyAsync(&status, P.status, sizeof status, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(off, P.out_offsets, sizeof off, hipMemcpyDeviceToHost, c->stream));
    if (opt) HIPCHK(c, hipMemcpyAsync(specs, P.specs, sizeof specs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (status & 1u) return HVC_E_RANGE;
    if ((status & 6u) || off[1] > seg_cap) return HVC_E_TOO_LARGE;
    hvc::jpeg_header_bytes(&info, header, opt ? specs : nullptr, ri);
    *out_len = header.size() + (size_t)off[1] + 2;
    if (!out || *out_len > cap) return HVC_E_INVALID_ARG;
    std::memcpy(out, header.data(), header.size());
    HIPCHK(c, hipMemcpy(out + header.size(), c->hd_out.p, (size_t)off[1], hipMemcpyDeviceToHost));
    out[header.size() + off[1]] = 0xff; // complete_and_write_eoi (encoder.ml:507-510)
    out[header.size() + off[1] + 1] = 0xd9;
    return HVC_OK;
}

hipError_t rgb_to_ycc_libjpeg_device(const uint8_t *d_rgb, const RgbImage &im, int width, int height, int sampling, int n_frames, uint8_t *d_yuv,
                                     size_t yuv_fs, const hvc_component *comps, bool pad, hipStream_t s) {
    if (n_frames <= 0 || width <= 0 || height <= 0) return hipSuccess;
    const bool grey = sampling == HVC_YUV_400;
    hvc::RgbLibjpegParams P;
    std::memset(&P, 0, sizeof P);
    P.rgb = d_rgb;
    P.yuv = d_yuv;
    P.rgb_fs = im.frame_stride;
    P.yuv_fs = yuv_fs;
    P.n_frames = n_frames;
    P.planar = im.layout == HVC_RGB_PLANAR;
    P.pad = pad;
    hvc::MixedRgbImageK &K = P.image;
    K.y_base = comps[0].plane_offset;
    K.y_stride = comps[0].stride;
    if (!grey) {
        K.cb_base = comps[1].plane_offset, K.cr_base = comps[2].plane_offset;
        K.cb_stride = comps[1].stride, K.cr_stride = comps[2].stride;
    }
    K.row_stride = im.row_stride;
    K.plane_stride = im.row_stride * (size_t)height;
    K.w = width, K.h = height;
    K.cw = sampling == HVC_YUV_444 ? width : width / 2, K.ch = sampling == HVC_YUV_420 ? height / 2 : height;
    K.sampling = sampling;
    unsigned lx, ly;
    hvc::libjpeg_rgb_lane_grid(width, height, sampling, pad, lx, ly);
    if ((unsigned long long)lx * ly * lx >= (1ull << 32)) return hipErrorInvalidValue; // (the lane's row by a reciprocal; 65535 x 65535 stays far inside)
    K.groups = lx;
    K.magic = lx > 1 ? (unsigned)(((1ull << 32) + lx - 1) / lx) : 0u;
    K.lanes = lx * ly;
    return hvc::launch_rgb_to_ycc_libjpeg(P, s);
}

// hvc_jpeg_encode of the planes the colour pass makes of an RGB image: the image goes up as it is, k_rgb_to_ycc writes the
// frame's samples into zeroed padded planes (Plane.create + blit_available), the rest is hvc_jpeg_encode's.
int hvc_jpeg_encode_rgb(hvc_ctx *c, const uint8_t *rgb, size_t rgb_row_stride, int layout, int width, int height, int chroma, int quality,
                        uint8_t *out, size_t cap, size_t *out_len) try {
    if (!c || !rgb || !out_len) return HVC_E_INVALID_ARG;
    hvc_jpeg_info info;
    int r = hvc_jpeg_encoder_layout(width, height, chroma, quality, &info);
    if (r) return r;
    if ((r = hvc_jpeg_encoder_check(&info))) return r; // the model raises for this geometry
    if (((chroma == 420 || chroma == 422) && (width & 1)) || (chroma == 420 && (height & 1))) return HVC_E_INVALID_ARG; // Yuv.assert_is_420 / _422
    RgbImage im;
    if (!rgb_image(layout, width, height, rgb_row_stride, 0, im)) return HVC_E_INVALID_ARG;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    size_t seg_cap = 0;
    if ((r = encode_scratch(c, info, &seg_cap))) return r;
    const size_t in_bytes = rgb_bytes(im, 1);
    if ((r = grow(c, c->d_aux2, in_bytes))) return r;
    HIPCHK(c, hipMemcpyAsync(c->d_aux2.p, rgb, in_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_in.p, 0, info.pixel_bytes, c->stream));
    // hvc_set_encode_libjpeg: libjpeg's averaging, and the replicated edge written by the colour pass itself (the clear stays: the
    // samples of the dummy blocks are never looked at)
    HIPCHK(c, c->enc_libjpeg ? rgb_to_ycc_libjpeg_device(c->d_aux2.as<const uint8_t>(), im, width, height, chroma, 1, c->d_in.as<uint8_t>(),
                                                         info.pixel_bytes, info.layout, true, c->stream)
                             : rgb_to_ycc_device(c->d_aux2.as<const uint8_t>(), im, width, height, chroma, 1, c->d_in.as<uint8_t>(),
                                                 info.pixel_bytes, info.layout, c->stream));
    return encode_padded_on_device(c, info, seg_cap, out, cap, out_len);
} HVC_ABI_CATCH

// ---------------------------------------------------------------------------
// BASELINE config 3: host Huffman || hipMemcpyAsync (copy stream) || block-stage kernel (compute stream)

// form: what every frame's records become (OutputForm, hvc_ctx.h) -- a file whose DC leaves int16 is HVC_E_RANGE in a scaled batch
int decode_batch_impl(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int threads,
                             int frames_per_chunk, uint8_t *pixels, size_t pixel_fs, int where, hvc_batch_stats *stats,
                             OutputForm form) {
    if (!c || !jpegs || !sizes || !pixels || n_frames < 0) return HVC_E_INVALID_ARG;
    if (!form.known()) return HVC_E_INVALID_ARG;
    if (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE) return HVC_E_INVALID_ARG;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_frames == 0) return HVC_OK;
    hvc::RestartScope honour(c->honour_restart);
    hvc_jpeg_info info0;
    int r = hvc_jpeg_read_header(jpegs[0], sizes[0], &info0);
    if (r) return r;
    form.of(info0);
    if ((r = form.batch_check(pixel_fs))) return r;
    const size_t out_bytes = form.out_bytes; // per frame
    if (info0.coef_count == 0) { // frames without a block (a width or height of zero): nothing to upload, nothing to launch --
        for (int f = 0; f < n_frames; f++) { // every file is still read as the model reads it (headers, tables)
            hvc_jpeg_info fi;
            if ((r = hvc_jpeg_read_header(jpegs[f], sizes[f], &fi))) return r;
            if (fi.n_comp != info0.n_comp || fi.coef_count != 0 || std::memcmp(fi.layout, info0.layout, sizeof fi.layout)) return HVC_E_INVALID_ARG;
            if ((r = hvc_jpeg_entropy_decode(jpegs[f], sizes[f], &fi, nullptr))) return r;
        }
        return HVC_OK;
    }
    if (threads < 1) threads = 1;
    if (threads > 256) threads = 256;
    if (frames_per_chunk < 1) frames_per_chunk = 32;
    if (frames_per_chunk > n_frames) frames_per_chunk = n_frames;
    const int C = frames_per_chunk, NB = hvc_ctx::RING;
    const int n_chunks = (n_frames + C - 1) / C;
    const size_t frame_coef_bytes = info0.coef_count * sizeof(int16_t);
    const size_t ring_bytes = frame_coef_bytes * (size_t)C;
    const size_t oring_bytes = where == HVC_MEM_HOST ? out_bytes * (size_t)C : 0;

    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    if ((r = pipeline_events(c))) return r;
    if ((r = ring_ensure(c, coef_rings(c), {ring_bytes, ring_bytes}))) return r;
    if ((r = ring_ensure(c, out_rings(c), {oring_bytes}))) return r;

    // worker threads pull frames in order; a frame's chunk slot must have been released (its previous
    // occupant uploaded) before they write into it
    std::vector<std::vector<WideFix>> chunk_wide((size_t)n_chunks); // blocks whose DC left int16 (frame = index in the chunk)
    std::atomic<long long> entropy_ns{0};
    const auto wall0 = std::chrono::steady_clock::now();
    if ((r = pool_ready(c, threads))) return r;
    hvc::ChunkFeed feed(c->pool, n_chunks, NB); // (after everything a pool task touches)
    auto worker = [&]() {
        if (!pin_to_ctx_cpus(c)) feed.raise(HVC_E_INVALID_ARG); // hvc_set_host_cpus
        hvc::RestartScope honour(c->honour_restart); // (a pool thread reads the files: the flag is its own)
        // Frames are taken TWO at a time and decoded symbol by symbol in turn (hvc::entropy_decode_wide2): one stream is
        // one dependency chain, two streams are two chains the core overlaps -- 1.4x the frames per second per thread.
        std::vector<hvc::WideDc> wide2[2];
        static const int take = [] { const char *v = std::getenv("HVC_HOST_PAIRS"); return v && v[0] == '0' ? 1 : 2; }(); // (A/B: 0 = one file at a time)
        for (;;) {
            const int f0 = feed.claim(take);
            if (f0 >= n_frames || feed.error()) return;
            const int cnt = (take == 2 && f0 + 1 < n_frames) ? 2 : 1;
            if (!feed.wait_slot((f0 + cnt - 1) / C)) return;
            const auto t0 = std::chrono::steady_clock::now();
            hvc_jpeg_info fi[2];
            int e[2] = {HVC_OK, HVC_OK};
            int16_t *dst[2] = {nullptr, nullptr};
            for (int q = 0; q < cnt; q++) {
                const int f = f0 + q, k = f / C;
                e[q] = hvc_jpeg_read_header(jpegs[f], sizes[f], &fi[q]);
                if (!e[q] && (fi[q].n_comp != info0.n_comp || fi[q].n_qtabs != info0.n_qtabs || fi[q].coef_count != info0.coef_count ||
                              std::memcmp(fi[q].layout, info0.layout, sizeof fi[q].layout) ||
                              std::memcmp(fi[q].qtabs, info0.qtabs, sizeof fi[q].qtabs)))
                    e[q] = HVC_E_INVALID_ARG; // a batch shares one geometry and one set of tables
                dst[q] = c->h_ring[k % NB].as<int16_t>() + (size_t)(f - k * C) * info0.coef_count;
            }
            if (cnt == 2 && !e[0] && !e[1]) {
                const uint8_t *const data[2] = {jpegs[f0], jpegs[f0 + 1]};
                const size_t len[2] = {sizes[f0], sizes[f0 + 1]};
                const hvc_jpeg_info *const inf[2] = {&fi[0], &fi[1]};
                std::vector<hvc::WideDc> *const wd[2] = {&wide2[0], &wide2[1]};
                hvc::entropy_decode_wide2(data, len, inf, dst, wd, e);
            } else {
                for (int q = 0; q < cnt; q++)
                    if (!e[q]) e[q] = hvc::entropy_decode_wide(jpegs[f0 + q], sizes[f0 + q], &fi[q], dst[q], wide2[q]);
            }
            entropy_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
            for (int q = 0; q < cnt; q++) { // (the pair's first error: frame order)
                const int f = f0 + q, k = f / C;
                if (!e[q] && !wide2[q].empty()) {
                    std::lock_guard<std::mutex> lk(feed.mutex());
                    try {
                        for (const hvc::WideDc &w : wide2[q]) chunk_wide[(size_t)k].push_back(WideFix{f - k * C, w.block, w.dc});
                    } catch (const std::bad_alloc &) {
                        e[q] = HVC_E_OUT_OF_MEMORY;
                    }
                }
                feed.report(k, 1, e[q]);
            }
        }
    };
    if ((r = feed.start(threads, worker))) return r;

    auto first_of = [&](int k) { return k * C; };
    auto count_of = [&](int k) { return first_of(k) + C <= n_frames ? C : n_frames - first_of(k); };
    auto dst_of = [&](int k, int slot) { return where == HVC_MEM_DEVICE ? pixels + (size_t)first_of(k) * pixel_fs : c->d_oring[slot].as<uint8_t>(); };
    const size_t dst_fs = where == HVC_MEM_DEVICE ? pixel_fs : out_bytes;
    r = host_reader_chunks(
        c, feed, n_chunks, threads, wall0, count_of, [&](int k) { return frame_coef_bytes * (size_t)count_of(k); },
        [&](int k, int slot) {
            DecodeOpts o(c);
            o.profile = form.chunk_profile(c);
            o.wide = &chunk_wide[(size_t)k]; // (complete: the chunk's workers are done)
            return form.run(c, c->d_ring[slot].as<const int16_t>(), count_of(k), dst_of(k, slot), dst_fs, HVC_MEM_DEVICE, o);
        },
        [&](int k, int slot) {
            hipError_t he = hipSuccess;
            for (int f = 0; f < count_of(k) && he == hipSuccess && where == HVC_MEM_HOST; f++)
                he = hipMemcpyAsync(pixels + (size_t)(first_of(k) + f) * pixel_fs, dst_of(k, slot) + (size_t)f * dst_fs, out_bytes,
                                    hipMemcpyDeviceToHost, c->stream);
            return he;
        },
        stats);
    if (stats) {
        stats->entropy_ms_sum = (double)entropy_ns.load() * 1e-6;
        stats->frames_per_chunk = C;
        stats->coef_bytes = (uint64_t)frame_coef_bytes * (uint64_t)n_frames;
    }
    return r;
}

int hvc_jpeg_decode_batch(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int threads,
                          int frames_per_chunk, uint8_t *pixels, size_t pixel_fs, int where, hvc_batch_stats *stats) try {
    return decode_batch_impl(c, jpegs, sizes, n_frames, threads, frames_per_chunk, pixels, pixel_fs, where, stats,
                             OutputForm(OutputForm::PLANES));
} HVC_ABI_CATCH

// where the pixel record of every file of a mixed batch goes (host only: hvc_mixed_plan.cpp)
int hvc_jpeg_mixed_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, size_t align, hvc_jpeg_info *infos,
                          int *status, size_t *pixel_offsets, size_t *total_bytes) try {
    return hvc::mixed_layout(jpegs, sizes, n_files, align, infos, status, pixel_offsets, total_bytes);
} HVC_ABI_CATCH

// files of different sizes, samplings and tables in one call: hvc_capi_mixed.hip
int hvc_jpeg_decode_batch_mixed(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, int threads,
                                size_t chunk_bytes, const hvc_jpeg_info *infos, int *status, const size_t *pixel_offsets,
                                uint8_t *pixels, size_t pixel_cap, int where, hvc_batch_stats *stats) try {
    return decode_batch_mixed_impl(c, jpegs, sizes, n_files, threads, chunk_bytes, infos, status, pixel_offsets, pixels, pixel_cap,
                                   where, stats);
} HVC_ABI_CATCH

// who reads the files of the mixed batch calls (hvc_capi_mixed.hip, hvc_capi_mixed_reader.hip), and the last call's split
int hvc_set_mixed_reader(hvc_ctx *c, int which) try {
    if (!c || (which != HVC_READER_HOST && which != HVC_READER_GPU)) return HVC_E_INVALID_ARG;
    c->mixed_reader = which;
    return HVC_OK;
} HVC_ABI_CATCH

int hvc_get_mixed_reader(const hvc_ctx *c, int *which) try {
    if (!c || !which) return HVC_E_INVALID_ARG;
    *which = c->mixed_reader;
    return HVC_OK;
} HVC_ABI_CATCH

int hvc_last_mixed_reader_files(const hvc_ctx *c, uint64_t *gpu_files, uint64_t *host_files) try {
    if (!c) return HVC_E_INVALID_ARG;
    if (gpu_files) *gpu_files = c->mixed_gpu_files;
    if (host_files) *host_files = c->mixed_host_files;
    return HVC_OK;
} HVC_ABI_CATCH

// the mixed counterpart of hvc_jpeg_entropy_decode_gpu: hvc_capi_mixed_reader.hip
int hvc_jpeg_entropy_decode_gpu_mixed(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, const hvc_jpeg_info *infos,
                                      int *status, int16_t *coefs, const size_t *coef_offsets, size_t coef_cap, int where, int *used_gpu) try {
    return entropy_decode_gpu_mixed_impl(c, jpegs, sizes, n_files, infos, status, coefs, coef_offsets, coef_cap, where, used_gpu);
} HVC_ABI_CATCH

// ... at 1/2, 1/4, 1/8 size: the layout of the scaled records and the same pipeline with k_decode_mixed_scaled as its block
// stage; scale_denom = 1 is the full-size entry point itself
int hvc_jpeg_mixed_scaled_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int scale_denom, size_t align,
                                 hvc_jpeg_info *infos, hvc_jpeg_info *scaled, int *status, size_t *pixel_offsets, size_t *total_bytes) try {
    return hvc::mixed_scaled_layout(jpegs, sizes, n_files, scale_denom, align, infos, scaled, status, pixel_offsets, total_bytes);
} HVC_ABI_CATCH

int hvc_jpeg_decode_batch_mixed_scaled(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, int threads,
                                       size_t chunk_bytes, int scale_denom, const hvc_jpeg_info *infos, int *status,
                                       const size_t *pixel_offsets, uint8_t *pixels, size_t pixel_cap, int where, hvc_batch_stats *stats) try {
    if (!scaled_side(scale_denom)) return HVC_E_INVALID_ARG;
    MixedForm form;
    form.scale_denom = scale_denom;
    return decode_batch_mixed_impl(c, jpegs, sizes, n_files, threads, chunk_bytes, infos, status, pixel_offsets, pixels, pixel_cap,
                                   where, stats, form);
} HVC_ABI_CATCH

int hvc_jpeg_mixed_scaled_rgb_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int scale_denom, int layout,
                                     size_t align, size_t row_align, hvc_jpeg_info *infos, hvc_jpeg_info *scaled, int *status,
                                     size_t *rgb_offsets, size_t *rgb_row_strides, size_t *total_bytes) try {
    return hvc::mixed_scaled_rgb_layout(jpegs, sizes, n_files, scale_denom, layout, align, row_align, infos, scaled, status, rgb_offsets,
                                        rgb_row_strides, total_bytes);
} HVC_ABI_CATCH

int hvc_jpeg_decode_batch_mixed_scaled_rgb(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, int threads,
                                           size_t chunk_bytes, int scale_denom, const hvc_jpeg_info *infos, int *status,
                                           const size_t *rgb_offsets, const size_t *rgb_row_strides, uint8_t *rgb, size_t rgb_cap,
                                           int layout, int where, hvc_batch_stats *stats) try {
    if (!scaled_side(scale_denom) || !rgb_offsets) return HVC_E_INVALID_ARG;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    MixedForm form;
    form.rgb_offsets = rgb_offsets;
    form.rgb_row_strides = rgb_row_strides;
    form.layout = layout;
    form.scale_denom = scale_denom;
    return decode_batch_mixed_impl(c, jpegs, sizes, n_files, threads, chunk_bytes, infos, status, rgb_offsets, rgb, rgb_cap, where, stats, form);
} HVC_ABI_CATCH

// ... to RGB images: where every file's image goes (host only: hvc_mixed_rgb_plan.cpp), and the pipeline with the colour pass
// behind every chunk's block stage
int hvc_jpeg_mixed_rgb_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int layout, size_t align, size_t row_align,
                              hvc_jpeg_info *infos, int *status, size_t *rgb_offsets, size_t *rgb_row_strides, size_t *total_bytes) try {
    return hvc::mixed_rgb_layout(jpegs, sizes, n_files, layout, align, row_align, infos, status, rgb_offsets, rgb_row_strides, total_bytes);
} HVC_ABI_CATCH
int hvc_jpeg_decode_batch_mixed_rgb(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, int threads,
                                    size_t chunk_bytes, const hvc_jpeg_info *infos, int *status, const size_t *rgb_offsets,
                                    const size_t *rgb_row_strides, uint8_t *rgb, size_t rgb_cap, int layout, int where,
                                    hvc_batch_stats *stats) try {
    if (!rgb_offsets || (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR)) return HVC_E_INVALID_ARG;
    MixedForm form;
    form.rgb_offsets = rgb_offsets, form.rgb_row_strides = rgb_row_strides, form.layout = layout;
    return decode_batch_mixed_impl(c, jpegs, sizes, n_files, threads, chunk_bytes, infos, status, rgb_offsets, rgb, rgb_cap, where, stats, form);
} HVC_ABI_CATCH

// ... ending in the two resampling passes: every image to the size the caller names for it (hvc_capi_resize.hip); opts: a box
// and a mirror flag per file, a typed output (NULL or all zero: none of them)
int hvc_jpeg_decode_batch_mixed_resized_opts(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, int threads,
                                             size_t chunk_bytes, int scale_denom, const hvc_jpeg_info *infos, int *status, const int *out_widths,
                                             const int *out_heights, const size_t *dst_offsets, const size_t *dst_row_strides, uint8_t *dst,
                                             size_t dst_cap, int layout, int filter, int where, hvc_batch_stats *stats,
                                             const hvc_resize_opts *opts) try {
    if (!scaled_side(scale_denom) || !dst_offsets || !out_widths || !out_heights) return HVC_E_INVALID_ARG;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (filter != HVC_RESIZE_BOX && filter != HVC_RESIZE_BILINEAR && filter != HVC_RESIZE_BICUBIC) return HVC_E_INVALID_ARG;
    if (resize_opts_check(opts)) return HVC_E_INVALID_ARG;
    MixedForm form;
    form.rgb_offsets = dst_offsets, form.rgb_row_strides = dst_row_strides, form.layout = layout, form.scale_denom = scale_denom;
    form.out_widths = out_widths, form.out_heights = out_heights, form.filter = filter;
    if (opts) form.boxes = opts->boxes, form.mirror = opts->mirror, form.out_elem = opts->out_elem, form.lut = opts->lut;
    return decode_batch_mixed_impl(c, jpegs, sizes, n_files, threads, chunk_bytes, infos, status, dst_offsets, dst, dst_cap, where, stats, form);
} HVC_ABI_CATCH
int hvc_jpeg_decode_batch_mixed_resized(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, int threads,
                                        size_t chunk_bytes, int scale_denom, const hvc_jpeg_info *infos, int *status, const int *out_widths,
                                        const int *out_heights, const size_t *dst_offsets, const size_t *dst_row_strides, uint8_t *dst,
                                        size_t dst_cap, int layout, int filter, int where, hvc_batch_stats *stats) try {
    return hvc_jpeg_decode_batch_mixed_resized_opts(c, jpegs, sizes, n_files, threads, chunk_bytes, scale_denom, infos, status, out_widths,
                                                    out_heights, dst_offsets, dst_row_strides, dst, dst_cap, layout, filter, where, stats, nullptr);
} HVC_ABI_CATCH

int hvc_jpeg_decode_batch_yuv444(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames,
                                 int threads, int frames_per_chunk, uint8_t *frames, size_t frame_stride, int where,
                                 hvc_batch_stats *stats) try {
    if (c && c->arith != HVC_ARITH_MODEL) return HVC_E_INVALID_ARG; // (no RTL form of the fused path: hvc_set_arithmetic)
    return decode_batch_impl(c, jpegs, sizes, n_frames, threads, frames_per_chunk, frames, frame_stride, where, stats,
                             OutputForm(OutputForm::YUV444));
} HVC_ABI_CATCH

// hvc_jpeg_decode_batch_rgb: the batch pipelines as they are (host reader or GPU reader, whichever `gpu_reader` names), their
// planes into the context's scratch instead of the caller's memory, and the colour pass (hvc_rgb.hip) from there to where the
// output goes, on the same stream -- in parts of at most ~4 GB of planes, so that the scratch stays bounded whatever the batch.
int hvc_jpeg_decode_batch_rgb(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_frames, int threads, int frames_per_chunk,
                              int gpu_reader, uint8_t *rgb, size_t rgb_row_stride, size_t rgb_frame_stride, int layout, int where,
                              hvc_batch_stats *stats) try {
    if (!c || !jpegs || !sizes || !rgb || n_frames < 0) return HVC_E_INVALID_ARG;
    if (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE) return HVC_E_INVALID_ARG;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_frames == 0) return HVC_OK;
    if (!jpegs[0]) return HVC_E_INVALID_ARG;
    hvc_jpeg_info info0;
    int r = hvc_jpeg_read_header(jpegs[0], sizes[0], &info0);
    if (r) return r;
    const int sampling = rgb_sampling_of(info0);
    RgbImage im;
    if (!sampling || !rgb_image(layout, info0.width, info0.height, rgb_row_stride, rgb_frame_stride, im)) return HVC_E_INVALID_ARG;
    const bool empty = info0.width == 0 || info0.height == 0 || info0.pixel_bytes == 0;
    int cw, ch;
    rgb_chroma_window(sampling, info0.width, info0.height, cw, ch);
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    const size_t px_fs = info0.pixel_bytes;
    const int part = empty ? n_frames : (int)std::max<size_t>(1, std::min<size_t>((size_t)n_frames, ((size_t)4 << 30) / px_fs));
    if ((r = grow(c, c->d_aux, empty ? 8 : (size_t)part * px_fs))) return r;
    uint8_t *d_rgb = rgb;
    if (where == HVC_MEM_HOST && !empty) {
        if ((r = grow(c, c->d_aux2, rgb_bytes(im, part)))) return r;
        d_rgb = c->d_aux2.as<uint8_t>();
    }
    const auto wall0 = std::chrono::steady_clock::now();
    for (int f0 = 0; f0 < n_frames; f0 += part) {
        const int cnt = std::min(part, n_frames - f0);
        hvc_batch_stats ps;
        r = gpu_reader ? hvc_jpeg_decode_batch_gpu(c, jpegs + f0, sizes + f0, cnt, threads, frames_per_chunk, c->d_aux.as<uint8_t>(), px_fs,
                                                   HVC_MEM_DEVICE, 0, &ps)
                       : hvc_jpeg_decode_batch(c, jpegs + f0, sizes + f0, cnt, threads, frames_per_chunk, c->d_aux.as<uint8_t>(), px_fs,
                                               HVC_MEM_DEVICE, &ps);
        if (r) return r;
        if (stats) {
            stats->entropy_ms_sum += ps.entropy_ms_sum, stats->h2d_ms_sum += ps.h2d_ms_sum, stats->kernel_ms_sum += ps.kernel_ms_sum;
            stats->d2h_ms_sum += ps.d2h_ms_sum, stats->host_prep_ms_sum += ps.host_prep_ms_sum;
            stats->chunks += ps.chunks, stats->threads = ps.threads, stats->frames_per_chunk = ps.frames_per_chunk;
            stats->coef_bytes += ps.coef_bytes;
        }
        if (empty) continue;
        uint8_t *out = where == HVC_MEM_HOST ? d_rgb : d_rgb + (size_t)f0 * im.frame_stride;
        HIPCHK(c, ycc_to_rgb_device(c->d_aux.as<const uint8_t>(), px_fs, info0.layout, sampling, info0.width, info0.height, cw, ch, cnt, out, im,
                                    c->stream, c->arith));
        if (where == HVC_MEM_HOST) {
            HIPCHK(c, rgb_download(out, rgb + (size_t)f0 * im.frame_stride, im, cnt, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    if (stats) stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return HVC_OK;
} HVC_ABI_CATCH
