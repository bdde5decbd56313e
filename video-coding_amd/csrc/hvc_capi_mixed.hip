// hvc_capi_mixed.hip -- batches of frames (behind hvc_decode_frames_mixed) and of files (behind hvc_jpeg_decode_batch_mixed) that share
// neither geometry nor quantiser tables: the host plan of hvc_mixed_plan.cpp, its tables in device memory, one launch of
// k_decode_mixed (hvc_mixed.hip) per call or per chunk.  The pipeline reuses the context's pinned / device rings, events and
// worker pool of hvc_jpeg_decode_batch; what it cuts the batch by is bytes, not frames.  The RGB forms (hvc_yuv_to_rgb_mixed,
// hvc_decode_frames_mixed_rgb, hvc_jpeg_decode_batch_mixed_rgb) put one launch of k_ycc_to_rgb_mixed (hvc_mixed_rgb.hip) behind
// the planes, from the host plan of hvc_mixed_rgb_plan.cpp.
// The reduced-size forms (hvc_decode_frames_mixed_scaled, hvc_jpeg_decode_batch_mixed_scaled, _scaled_rgb) are the same code with the
// plan built for N = 8 / scale_denom samples per block side and k_decode_mixed_scaled (hvc_mixed_scaled.hip) as the block stage.
#include "hvc_batch.h"
#include "hvc_mixed.h"
#include "hvc_mixed_libjpeg.h"
#include "hvc_mixed_rgb.h"
#include "hvc_mixed_reader.h"
#include "hvc_resize_plan.h"

// A plan's image in a device buffer of the context, in stream order: uploaded from the pinned copy unless the device
// already holds these bytes.  (hvc_ctx.h: the mixed encode plans use it too)
int upload_image(hvc_ctx *c, PlanBuf &b, const std::vector<unsigned char> &img) {
    const size_t total = img.size();
    HIPCHK(c, b.ev.ensure(hipEventDisableTiming));
    const bool same = b.len == total && b.h && !std::memcmp(b.h.p, img.data(), total);
    if (same) return HVC_OK;
    b.len = 0;
    int r = grow(c, b.d, total);
    if (r) return r;
    if (total > b.h.cap) {
        if ((r = grow(c, b.h, total, GROW_PLAN_IMAGE))) return r;
    } else {
        HIPCHK(c, wait_event(b.ev)); // (the last upload has read the image)
    }
    std::memcpy(b.h.p, img.data(), total);
    HIPCHK(c, hipMemcpyAsync(b.d.p, b.h.p, total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(b.ev, c->stream));
    b.len = total;
    return HVC_OK;
}

// ... made of `parts` one after another, each on 16 bytes: at[i] = where part i starts in the image
int upload_parts(hvc_ctx *c, PlanBuf &b, std::initializer_list<ImagePart> parts, size_t *at) {
    size_t total = 0, i = 0;
    for (const ImagePart &p : parts) at[i++] = total, total += (p.bytes + 15) & ~(size_t)15;
    std::vector<unsigned char> img(total, 0);
    i = 0;
    for (const ImagePart &p : parts) {
        if (p.bytes) std::memcpy(img.data() + at[i], p.p, p.bytes);
        i++;
    }
    return upload_image(c, b, img);
}

namespace {

// the block stage's tables in c->mixed_plan, planes | tables | map | pairs; pairs (optional): the libjpeg-exact block stage's
// table records (mixed_islow_pairs_build) -- none under the model's arithmetic, whose image is the first three parts and
// nothing else; *d_pairs = where they are on the device
int upload_plan(hvc_ctx *c, const hvc::MixedPlan &plan, hvc::MixedParams &P, const std::vector<unsigned> *pairs = nullptr,
                const unsigned **d_pairs = nullptr) {
    size_t at[4];
    const int r = upload_parts(c, c->mixed_plan,
                               {{plan.planes.data(), plan.planes.size() * sizeof(hvc::MixedPlaneK)},
                                {plan.tables.data(), plan.tables.size() * sizeof(hvc::MixedTableK)},
                                {plan.map.data(), plan.map.size() * sizeof(unsigned)},
                                {pairs ? pairs->data() : nullptr, pairs ? pairs->size() * sizeof(unsigned) : 0}}, at);
    if (r) return r;
    const unsigned char *d = c->mixed_plan.d.as<const unsigned char>();
    P.planes = reinterpret_cast<const hvc::MixedPlaneK *>(d + at[0]);
    P.tables = reinterpret_cast<const hvc::MixedTableK *>(d + at[1]);
    P.map = reinterpret_cast<const unsigned *>(d + at[2]);
    P.n_units = (unsigned)plan.map.size();
    if (d_pairs) *d_pairs = reinterpret_cast<const unsigned *>(d + at[3]);
    return HVC_OK;
}

} // namespace

// The colour pass of a plan on DEVICE memory, enqueued on c->stream: its tables (images | map, each part on 16 bytes) go to
// c->mixed_rgb_plan, a buffer of their own.  to_ycc: the way back, k_rgb_to_ycc_mixed over a plan of
// mixed_rgb_encode_plan_build -- d_rgb is read, the planes at d_yuv are written (hvc_capi_mixed_encode.hip).
int mixed_rgb_launch_plan(hvc_ctx *c, const hvc::MixedRgbPlan &plan, int layout, const uint8_t *d_yuv, uint8_t *d_rgb, bool profile,
                          bool to_ycc) {
    if (plan.map.empty()) return HVC_OK; // no pixel at all: nothing to launch
    size_t at[2];
    const int r = upload_parts(c, c->mixed_rgb_plan, {{plan.images.data(), plan.images.size() * sizeof(hvc::MixedRgbImageK)},
                                                      {plan.map.data(), plan.map.size() * sizeof(unsigned)}}, at);
    if (r) return r;
    hvc::MixedRgbParams P;
    std::memset(&P, 0, sizeof P);
    P.yuv = d_yuv;
    P.rgb = d_rgb;
    P.images = c->mixed_rgb_plan.d.as<const hvc::MixedRgbImageK>();
    P.map = reinterpret_cast<const unsigned *>(c->mixed_rgb_plan.d.as<const unsigned char>() + at[1]);
    P.n_units = (unsigned)plan.map.size();
    P.planar = layout == HVC_RGB_PLANAR;
    // hvc_set_mixed_arithmetic(HVC_ARITH_LIBJPEG): the planes -> RGB direction with libjpeg's fancy upsampling
    const bool fancy = !to_ycc && c->mixed_arith == HVC_ARITH_LIBJPEG;
    HIPCHK(c, profiled_launch(c, profile, [&](hipEvent_t k0, hipEvent_t k1) {
               return to_ycc  ? hvc::launch_rgb_to_ycc_mixed(P, c->stream, k0, k1)
                      : fancy ? hvc::launch_ycc_to_rgb_fancy_mixed(P, c->stream, k0, k1)
                              : hvc::launch_ycc_to_rgb_mixed(P, c->stream, k0, k1);
           }));
    return HVC_OK;
}

namespace {

// the fix-up list holds one id per block slot of the launch (every unit may send all 64 of its lanes)
int reserve_mixed_fix_list(hvc_ctx *c, size_t entries) { return grow(c, c->d_fix_list, entries * sizeof(unsigned)); }

// The block stage of a plan on DEVICE memory, enqueued on c->stream.  The caller has called wide_total_begin for the call
// this launch belongs to.  n = 4, 2, 1: a plan built for the scaled block stage with d_pixels as its pix_addr
// (k_decode_mixed_scaled: no fix-up list, the call's first launch clears the total its int64 branch adds to).
int mixed_launch_plan(hvc_ctx *c, const hvc::MixedPlan &plan, const int16_t *d_coefs, uint8_t *d_pixels, bool profile, int n = 8) {
    int r;
    if (plan.map.empty()) return HVC_OK; // no block at all: nothing to launch
    if (((uintptr_t)d_coefs & 15) || (n == 8 && ((uintptr_t)d_pixels & 7))) return HVC_E_ALIGNMENT;
    if (n == 8 && c->mixed_arith == HVC_ARITH_LIBJPEG) {
        // k_islow_mixed (hvc_mixed_libjpeg.hip): its int64 path runs in the same lane, so no fix-up list; the call's first launch
        // clears the total it adds to, as the scaled stage below; hvc_set_decode_kernel(ctx, 2) sends every block there
        std::vector<unsigned> pairs;
        hvc::mixed_islow_pairs_build(plan, pairs);
        hvc::MixedParams M;
        std::memset(&M, 0, sizeof M);
        hvc::MixedIslowParams P;
        std::memset(&P, 0, sizeof P);
        if ((r = upload_plan(c, plan, M, &pairs, &P.pairs))) return r;
        P.coefs = d_coefs;
        P.pixels = d_pixels;
        P.planes = M.planes;
        P.map = M.map;
        P.n_units = M.n_units;
        P.all_wide = c->decode_kernel == 2;
        HIPCHK(c, wide_total_for_adding(c, P.wide_total));
        if (P.all_wide) c->wide_host = (c->wide_host < 0 ? 0 : c->wide_host) + (long long)plan.blocks;
        HIPCHK(c, profiled_launch(c, profile, [&](hipEvent_t k0, hipEvent_t k1) { return hvc::launch_islow_mixed(P, c->stream, k0, k1); }));
        return HVC_OK;
    }
    if (n == 8 && (r = reserve_mixed_fix_list(c, plan.map.size() * HVC_MIXED_UNIT))) return r;
    hvc::MixedParams P;
    std::memset(&P, 0, sizeof P);
    if ((r = upload_plan(c, plan, P))) return r;
    P.coefs = d_coefs;
    P.pixels = d_pixels;
    if (n != 8) { // k_decode_mixed_scaled: the total alone
        HIPCHK(c, wide_total_for_adding(c, P.wide_total));
        HIPCHK(c, profiled_launch(c, profile, [&](hipEvent_t k0, hipEvent_t k1) { return hvc::launch_decode_mixed_scaled(P, n, c->stream, k0, k1); }));
        return HVC_OK;
    }
    P.all_wide = c->decode_kernel == 2;
    fix_assign(c, P);
    const hipError_t e = profiled_launch(c, profile, [&](hipEvent_t k0, hipEvent_t k1) { return hvc::launch_decode_mixed(P, c->stream, k0, k1); });
    if (e != hipSuccess) {
        fix_reset(c);
        return fail_hip(c, e);
    }
    fix_commit(c);
    return HVC_OK;
}

// ... of the listed frames: frames = indices into infos / the offset arrays (nullptr: 0 .. n_list - 1)
int mixed_launch(hvc_ctx *c, const int16_t *d_coefs, const size_t *coef_offsets, const hvc_jpeg_info *infos, const int *frames,
                 int n_list, uint8_t *d_pixels, const size_t *pixel_offsets, bool profile, int n = 8) {
    hvc::MixedPlan plan;
    const int r = hvc::mixed_plan_build(infos, coef_offsets, pixel_offsets, frames, n_list, plan, n, (uintptr_t)d_pixels);
    return r ? r : mixed_launch_plan(c, plan, d_coefs, d_pixels, profile, n);
}

// what a frame's records cover: elements of coefficients, bytes of pixels (0: no block); n samples per block side
void frame_spans(const hvc_jpeg_info &fi, size_t &coef_span, size_t &pixel_span, int n = 8) {
    coef_span = pixel_span = 0;
    for (int i = 0; i < fi.n_comp && i < 4; i++) {
        const hvc_component &k = fi.layout[i];
        if (k.blocks_w <= 0 || k.blocks_h <= 0) continue;
        coef_span = std::max(coef_span, k.coef_offset + (size_t)k.blocks_w * k.blocks_h * 64);
        pixel_span = std::max(pixel_span, k.plane_offset + ((size_t)k.blocks_h * n - 1) * k.stride + (size_t)k.blocks_w * n);
    }
}

// The tight placement of a set's records in device scratch, each on 64 bytes: d_coef (int16 elements) / d_pix (bytes) per
// frame, ptot = the bytes of all pixel records; coefs != nullptr (host memory): uploaded to c->d_in in that placement.
// pix_addr (the scaled block stage, n < 8; may be nullptr): where the caller's pixel record f starts -- its d_pix keeps that
// address modulo 64, so that the planes take the dword or byte stores they would take in the caller's own placement.
int stage_coefs(hvc_ctx *c, const int16_t *coefs, const size_t *coef_offsets, const hvc_jpeg_info *infos, int n_frames,
                std::vector<size_t> &d_coef, std::vector<size_t> &d_pix, size_t &ptot, int n = 8, const uintptr_t *pix_addr = nullptr) {
    d_coef.assign((size_t)n_frames, 0);
    d_pix.assign((size_t)n_frames, 0);
    std::vector<size_t> cspan((size_t)n_frames);
    size_t ctot = 0;
    ptot = 0;
    for (int f = 0; f < n_frames; f++) {
        size_t ps;
        frame_spans(infos[f], cspan[(size_t)f], ps, n);
        const size_t shift = pix_addr ? (size_t)(pix_addr[f] & 63) : 0;
        d_coef[(size_t)f] = ctot;
        d_pix[(size_t)f] = ptot + shift;
        ctot += (cspan[(size_t)f] + 63) & ~(size_t)63;
        ptot += (shift + ps + 63) & ~(size_t)63;
    }
    if (!coefs) return HVC_OK;
    const int r = grow(c, c->d_in, ctot * sizeof(int16_t));
    if (r) return r;
    for (int f = 0; f < n_frames; f++)
        if (cspan[(size_t)f])
            HIPCHK(c, hipMemcpyAsync(c->d_in.as<int16_t>() + d_coef[(size_t)f], coefs + coef_offsets[f], cspan[(size_t)f] * sizeof(int16_t),
                                     hipMemcpyHostToDevice, c->stream));
    return HVC_OK;
}

// the rows of the plan's images, device -> host, laid out alike on both sides apart from the record offsets: only the bytes
// written (rows that touch: one copy per image)
hipError_t download_images(const hvc::MixedRgbPlan &plan, int layout, const uint8_t *d_rgb, uint8_t *h_rgb, const size_t *h_offsets, hipStream_t s) {
    for (size_t i = 0; i < plan.images.size(); i++) {
        const hvc::MixedRgbImageK &k = plan.images[i];
        const size_t row = hvc::mixed_rgb_row_bytes(layout, k.w), rows = hvc::mixed_rgb_rows(layout, k.h);
        uint8_t *dst = h_rgb + h_offsets[plan.frame[i]];
        const uint8_t *src = d_rgb + k.rgb_base;
        const hipError_t e = k.row_stride == row ? hipMemcpyAsync(dst, src, row * rows, hipMemcpyDeviceToHost, s)
                                                 : hipMemcpy2DAsync(dst, k.row_stride, src, k.row_stride, row, rows, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace

// where the images of a host-memory call go in device scratch: one after another, each keeping its offset modulo 64 (the
// 8-byte paths then run for exactly the images a device-memory call with these offsets would take them for)
size_t stage_offsets(const size_t *offsets, const std::vector<size_t> &spans, std::vector<size_t> &d_off) {
    size_t tot = 0;
    d_off.assign(spans.size(), 0);
    for (size_t f = 0; f < spans.size(); f++) {
        d_off[f] = tot + (offsets[f] & 63);
        tot = (d_off[f] + spans[f] + 63) & ~(size_t)63;
    }
    return tot;
}

// behind hvc_decode_frames_mixed (hvc_capi.hip)
int decode_frames_mixed_impl(hvc_ctx *c, const int16_t *coefs, const size_t *coef_offsets, const hvc_jpeg_info *infos, int n_frames,
                             uint8_t *pixels, const size_t *pixel_offsets, int where, int scale_denom) {
    const int N = scaled_side(scale_denom);
    if (!c || !N || n_frames < 0 || (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE)) return HVC_E_INVALID_ARG;
    bool libjpeg;
    if (mixed_arith_of(c, scale_denom, libjpeg)) return HVC_E_INVALID_ARG; // (hvc_ctx.h: the rule of hvc_set_mixed_arithmetic)
    if (n_frames == 0) return HVC_OK;
    if (!infos || !coef_offsets || !pixel_offsets) return HVC_E_INVALID_ARG;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    int r;
    {
        hvc::MixedPlan plan; // the caller's own offsets: checked for either kind of memory, launched on for device memory
        if ((r = hvc::mixed_plan_build(infos, coef_offsets, pixel_offsets, nullptr, n_frames, plan, N, (uintptr_t)pixels))) return r;
        if (plan.map.empty()) return HVC_OK; // (a set without a block needs no memory)
        if (!coefs || !pixels) return HVC_E_INVALID_ARG;
        if (where == HVC_MEM_DEVICE) {
            wide_total_begin(c);
            return mixed_launch_plan(c, plan, coefs, pixels, c->profiling, N);
        }
    }
    // host memory: the frames' records one after another in c->d_in / c->d_out (whole 128-byte blocks: every alignment rule
    // holds), each plane's bytes copied back by themselves -- what the kernels wrote, never the caller's padding
    std::vector<size_t> d_coef, d_pix;
    std::vector<uintptr_t> h_pix; // (scaled: where the caller's records start)
    if (N != 8)
        for (int f = 0; f < n_frames; f++) h_pix.push_back((uintptr_t)pixels + pixel_offsets[f]);
    size_t ptot = 0;
    if ((r = stage_coefs(c, coefs, coef_offsets, infos, n_frames, d_coef, d_pix, ptot, N, N != 8 ? h_pix.data() : nullptr))) return r;
    if ((r = grow(c, c->d_out, ptot))) return r;
    wide_total_begin(c);
    if ((r = mixed_launch(c, c->d_in.as<const int16_t>(), d_coef.data(), infos, nullptr, n_frames, c->d_out.as<uint8_t>(), d_pix.data(), false, N))) {
        (void)hipStreamSynchronize(c->stream);
        return r;
    }
    for (int f = 0; f < n_frames; f++)
        for (int i = 0; i < infos[f].n_comp; i++) {
            const hvc_component &k = infos[f].layout[i];
            if (k.blocks_w <= 0 || k.blocks_h <= 0) continue;
            const size_t row = (size_t)k.blocks_w * N, rows = (size_t)k.blocks_h * N;
            uint8_t *dst = pixels + pixel_offsets[f] + k.plane_offset;
            const uint8_t *src = c->d_out.as<const uint8_t>() + d_pix[(size_t)f] + k.plane_offset;
            if (k.stride == row)
                HIPCHK(c, hipMemcpyAsync(dst, src, row * rows, hipMemcpyDeviceToHost, c->stream));
            else
                HIPCHK(c, hipMemcpy2DAsync(dst, k.stride, src, k.stride, row, rows, hipMemcpyDeviceToHost, c->stream));
        }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HVC_OK;
}

// what the three RGB entry points check alike; HVC_OK with nothing = true: an empty set
static int mixed_rgb_args(const hvc_ctx *c, const void *infos, const void *in_offsets, const void *rgb_offsets, int n_frames, int layout,
                          int where, bool &nothing) {
    if (!c || n_frames < 0 || (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE)) return HVC_E_INVALID_ARG;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    bool libjpeg;
    if (mixed_arith_of(c, 1, libjpeg)) return HVC_E_INVALID_ARG; // (as the mixed block stage)
    nothing = n_frames == 0;
    if (!nothing && (!infos || !in_offsets || !rgb_offsets)) return HVC_E_INVALID_ARG;
    return HVC_OK;
}

// the images' spans (bytes from the record's start to the last byte written) by the caller's row strides
static int rgb_spans(const hvc_jpeg_info *infos, const size_t *rgb_row_strides, int n_frames, int layout, std::vector<size_t> &spans) {
    spans.assign((size_t)n_frames, 0);
    for (int f = 0; f < n_frames; f++) {
        if (infos[f].width < 0 || infos[f].height < 0) return HVC_E_INVALID_ARG;
        const size_t tight = hvc::mixed_rgb_row_bytes(layout, infos[f].width);
        const size_t rs = rgb_row_strides && rgb_row_strides[f] ? rgb_row_strides[f] : tight;
        if (rs < tight) return HVC_E_INVALID_ARG;
        spans[(size_t)f] = hvc::mixed_rgb_span(layout, infos[f].width, infos[f].height, rs);
    }
    return HVC_OK;
}

// behind hvc_yuv_to_rgb_mixed (hvc_yuv.hip)
int yuv_to_rgb_mixed_impl(hvc_ctx *c, const uint8_t *yuv, const size_t *yuv_offsets, const hvc_jpeg_info *infos, int n_frames, uint8_t *rgb,
                          const size_t *rgb_offsets, const size_t *rgb_row_strides, int layout, int where) {
    bool nothing = false;
    int r = mixed_rgb_args(c, infos, yuv_offsets, rgb_offsets, n_frames, layout, where, nothing);
    if (r || nothing) return r;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    hvc::MixedRgbPlan plan; // the caller's own offsets: checked for either kind of memory, launched on for device memory
    if ((r = hvc::mixed_rgb_plan_build(infos, yuv_offsets, rgb_offsets, rgb_row_strides, layout, nullptr, n_frames, (uintptr_t)yuv,
                                       (uintptr_t)rgb, false, plan)))
        return r;
    if (plan.map.empty()) return HVC_OK; // (a set without a pixel needs no memory)
    if (!yuv || !rgb) return HVC_E_INVALID_ARG;
    if (where == HVC_MEM_DEVICE) return mixed_rgb_launch_plan(c, plan, layout, yuv, rgb, c->profiling);
    // host memory: the listed images' plane records and RGB images one after another in c->d_in / c->d_out
    std::vector<size_t> yspan((size_t)n_frames, 0), rspan, d_yuv, d_rgb;
    if ((r = rgb_spans(infos, rgb_row_strides, n_frames, layout, rspan))) return r;
    for (size_t i = 0; i < plan.images.size(); i++) {
        const hvc::MixedRgbImageK &k = plan.images[i];
        const int f = plan.frame[i];
        yspan[(size_t)f] = rgb_yuv_span(infos[f].layout, k.sampling, k.w, k.h, k.cw, k.ch);
    }
    for (int f = 0; f < n_frames; f++)
        if (!yspan[(size_t)f]) rspan[(size_t)f] = 0; // (no image: no room)
    const size_t ytot = stage_offsets(yuv_offsets, yspan, d_yuv), rtot = stage_offsets(rgb_offsets, rspan, d_rgb);
    if ((r = grow(c, c->d_in, ytot))) return r;
    if ((r = grow(c, c->d_out, rtot))) return r;
    if ((r = hvc::mixed_rgb_plan_build(infos, d_yuv.data(), d_rgb.data(), rgb_row_strides, layout, nullptr, n_frames, (uintptr_t)c->d_in.p,
                                       (uintptr_t)c->d_out.p, false, plan)))
        return r;
    for (int f = 0; f < n_frames; f++)
        if (yspan[(size_t)f])
            HIPCHK(c, hipMemcpyAsync(c->d_in.as<uint8_t>() + d_yuv[(size_t)f], yuv + yuv_offsets[f], yspan[(size_t)f], hipMemcpyHostToDevice, c->stream));
    if ((r = mixed_rgb_launch_plan(c, plan, layout, c->d_in.as<const uint8_t>(), c->d_out.as<uint8_t>(), false))) {
        (void)hipStreamSynchronize(c->stream);
        return r;
    }
    HIPCHK(c, download_images(plan, layout, c->d_out.as<const uint8_t>(), rgb, rgb_offsets, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HVC_OK;
}

// behind hvc_decode_frames_mixed_rgb (hvc_capi.hip): hvc_decode_frames_mixed into c->d_aux (tight records on 64 bytes), the
// colour pass from there; host memory: the images are staged in c->d_aux2
int decode_frames_mixed_rgb_impl(hvc_ctx *c, const int16_t *coefs, const size_t *coef_offsets, const hvc_jpeg_info *infos, int n_frames,
                                 uint8_t *rgb, const size_t *rgb_offsets, const size_t *rgb_row_strides, int layout, int where) {
    bool nothing = false;
    int r = mixed_rgb_args(c, infos, coef_offsets, rgb_offsets, n_frames, layout, where, nothing);
    if (r || nothing) return r;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    std::vector<size_t> d_coef, d_pix, rspan, d_rgb;
    size_t ptot = 0;
    if ((r = stage_coefs(c, nullptr, coef_offsets, infos, n_frames, d_coef, d_pix, ptot))) return r;
    if ((r = rgb_spans(infos, rgb_row_strides, n_frames, layout, rspan))) return r;
    const bool host = where == HVC_MEM_HOST;
    const size_t rtot = host ? stage_offsets(rgb_offsets, rspan, d_rgb) : 0;
    hvc::MixedPlan bplan; // both plans before anything is enqueued: a set that is refused leaves nothing behind
    hvc::MixedRgbPlan cplan;
    if ((r = hvc::mixed_plan_build(infos, host ? d_coef.data() : coef_offsets, d_pix.data(), nullptr, n_frames, bplan))) return r;
    if ((r = grow(c, c->d_aux, ptot))) return r;
    if (host && (r = grow(c, c->d_aux2, rtot))) return r;
    uint8_t *out = host ? c->d_aux2.as<uint8_t>() : rgb;
    if ((r = hvc::mixed_rgb_plan_build(infos, d_pix.data(), host ? d_rgb.data() : rgb_offsets, rgb_row_strides, layout, nullptr, n_frames,
                                       (uintptr_t)c->d_aux.p, (uintptr_t)out, true, cplan)))
        return r;
    if (bplan.map.empty()) return HVC_OK; // (no block: no pixel)
    if (!coefs || (!cplan.map.empty() && !rgb)) return HVC_E_INVALID_ARG;
    if (host && (r = stage_coefs(c, coefs, coef_offsets, infos, n_frames, d_coef, d_pix, ptot))) return r;
    wide_total_begin(c);
    r = mixed_launch_plan(c, bplan, host ? c->d_in.as<const int16_t>() : coefs, c->d_aux.as<uint8_t>(), !host && c->profiling);
    if (!r) r = mixed_rgb_launch_plan(c, cplan, layout, c->d_aux.as<const uint8_t>(), out, false);
    if (r) {
        (void)hipStreamSynchronize(c->stream);
        return r;
    }
    if (host) {
        HIPCHK(c, download_images(cplan, layout, out, rgb, rgb_offsets, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return HVC_OK;
}

// ---------------------------------------------------------------------------
// Files -> pixels: host Huffman reader || upload (copy stream) || k_decode_mixed of the previous chunk (compute stream), as
// decode_batch_impl (hvc_capi_jpeg.hip) -- with chunks cut by the bytes of their coefficient records, a plan per chunk, and a
// status per file: a file that fails keeps its slot in the chunk's ring buffer and is left out of the chunk's plan.
// Which files take part, every offset into a ring slot, the ring sizes and the copies that take a chunk's output back to host
// memory are hvc::MixedDecodeChunks (hvc_mixed_decode_chunks.cpp, plain C++): nothing below rounds, compares or bounds an offset.
// form.rgb(): a file's record in `pixels` is its RGB image; the chunk's planes go to a device slot of their own ring and
// k_ycc_to_rgb_mixed follows k_decode_mixed on the compute stream.  form.scale_denom = 2, 4, 8: the same pipeline with the
// scaled infos describing every output and k_decode_mixed_scaled as the block stage; full-size planes exist nowhere.
// form.resized(): a file's record in `pixels` is its image taken to the size the caller names; the colour pass writes the
// chunk's images, tight, into a device slot of the RGB ring and the two resampling passes (hvc_capi_resize.hip) follow it on
// the compute stream, through a slot of the intermediates' ring, into where the images would have gone.
// hvc_set_mixed_reader(HVC_READER_GPU) (and not host_reader_only): the workers only unstuff the files' segments into the pinned
// reader ring (MixedGpuReader::prepare), the copy stream uploads them with the chunk's descriptors and table records, and the
// mixed GPU Huffman reader writes the coefficient records into d_ring[slot] in front of the block stage, which runs over the
// files whose verdict is clean; chunks, coef_rel and everything from the coefficient slot on are the same.  The files the
// reader hands back are decoded by this function itself, host_reader_only, in one call once the chunks are through.
// (behind hvc_jpeg_decode_batch_mixed and hvc_jpeg_decode_batch_mixed_rgb, hvc_capi_jpeg.hip)
int decode_batch_mixed_impl(hvc_ctx *c, const uint8_t *const *jpegs, const size_t *sizes, int n_files, int threads,
                            size_t chunk_bytes, const hvc_jpeg_info *infos, int *status, const size_t *pixel_offsets,
                            uint8_t *pixels, size_t pixel_cap, int where, hvc_batch_stats *stats, const MixedForm &form,
                            bool host_reader_only) {
    if (c && !host_reader_only) c->mixed_gpu_files = c->mixed_host_files = 0;
    if (!c || !jpegs || !sizes || !infos || !status || !pixel_offsets || n_files < 0) return HVC_E_INVALID_ARG;
    if (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE) return HVC_E_INVALID_ARG;
    bool libjpeg;
    if (mixed_arith_of(c, form.scale_denom, libjpeg)) return HVC_E_INVALID_ARG; // (scaled forms under the libjpeg setting among them)
    const int N = scaled_side(form.scale_denom); // (0: the chunk plan refuses the form)
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (threads < 1) threads = 1;
    if (threads > 256) threads = 256;
    const int NB = hvc_ctx::RING;
    // the files that take part (their header was read), cut into chunks; everything else keeps the status it came with
    hvc::MixedDecodeChunks plan;
    int r = hvc::mixed_decode_chunks_build(infos, status, jpegs, pixel_offsets, pixel_cap, pixels != nullptr, n_files, chunk_bytes, where, form, plan);
    if (r || plan.take.empty()) return r;
    const std::vector<hvc::MixedDecodeChunk> &chunks = plan.chunks;
    const std::vector<int> &take = plan.take, &chunk_of = plan.chunk_of;
    const std::vector<size_t> &coef_rel = plan.coef_rel;
    const hvc_jpeg_info *const oinfos = plan.out_infos(infos); // what describes a file's OUTPUT: its info, or the scaled form of it
    const int n_chunks = (int)chunks.size(), n_take = (int)take.size();
    uint64_t coef_total = 0;

    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    if ((r = pipeline_events(c))) return r;
    if ((r = ring_ensure(c, coef_rings(c), {plan.coef_ring, plan.coef_ring}))) return r; // (a single file larger than chunk_bytes: the ring grows)
    if ((r = ring_ensure(c, out_rings(c), {plan.out_ring}))) return r;
    if ((r = ring_ensure(c, plane_rings(c), {plan.plane_ring}))) return r;
    if (form.resized() && (r = ring_ensure(c, resize_rings(c), {plan.rgb_ring, plan.mid_ring}))) return r;
    // the GPU reader: which files of a chunk it hands back (known once the chunk's verdict is read), how many it read
    const bool gpu = c->mixed_reader == HVC_READER_GPU && !host_reader_only;
    MixedGpuReader rd; // (before the feed: pool tasks use it)
    std::vector<char> back(gpu ? (size_t)n_files : 0, 0);
    unsigned long long gpu_files = 0;
    hipError_t gpu_upload_err = hipSuccess;
    if (gpu && (r = rd.begin(c, jpegs, sizes, infos, coef_rel.data(), take, plan.chunk_first, plan.chunk_count))) return r;

    std::atomic<long long> entropy_ns{0};
    const auto wall0 = std::chrono::steady_clock::now();
    if ((r = pool_ready(c, threads))) return r;
    hvc::ChunkFeed feed(c->pool, n_chunks, NB); // (after everything a pool task touches)
    auto worker = [&]() {
        if (!pin_to_ctx_cpus(c)) feed.raise(HVC_E_INVALID_ARG);
        hvc::RestartScope honour(c->honour_restart);
        std::vector<hvc::WideDc> wide;
        for (;;) {
            const int t = feed.claim();
            if (t >= n_take || feed.error()) return;
            const int f = take[(size_t)t], k = chunk_of[(size_t)f];
            if (!feed.wait_slot(k)) return;
            const auto t0 = std::chrono::steady_clock::now();
            if (gpu) { // the segment into the pinned reader ring; the file's result comes with its chunk's verdict
                rd.prepare(k, t);
                entropy_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
                feed.report(k, 1, HVC_OK);
                continue;
            }
            int e;
            if (infos[f].coef_count == 0) { // no block: the file is still read as the model reads it
                e = hvc_jpeg_entropy_decode(jpegs[f], sizes[f], &infos[f], nullptr);
            } else {
                wide.clear();
                e = hvc::entropy_decode_wide(jpegs[f], sizes[f], &infos[f], c->h_ring[k % NB].as<int16_t>() + coef_rel[(size_t)f], wide);
                if (!e && !wide.empty()) e = HVC_E_RANGE; // (a DC beyond int16: no side list here)
            }
            entropy_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
            status[f] = e; // the file's own result: it stops nobody else (read once the chunk is complete)
            feed.report(k, 1, HVC_OK);
        }
    };
    if ((r = feed.start(threads, worker))) return r;

    wide_total_begin(c);
    std::vector<int> ok; // the chunk's good files with blocks
    uint8_t *const out = where == HVC_MEM_DEVICE ? pixels : nullptr; // (host: the chunk's slot of d_oring)
    const size_t *dst_off = where == HVC_MEM_DEVICE ? pixel_offsets : plan.pix_rel.data();
    std::vector<hvc::MixedDecodeRun> runs; // the chunk's copies back to host memory
    r = host_reader_chunks(
        c, feed, n_chunks, threads, wall0, [&](int k) { return chunks[(size_t)k].count; },
        [&](int k) -> size_t {
            const hvc::MixedDecodeChunk &ch = chunks[(size_t)k];
            ok.clear();
            if (gpu) { // segments, descriptors, map and table records instead of coefficients (on the copy stream, as the copy would be)
                gpu_upload_err = rd.upload(k, c->copy_stream);
                coef_total += ch.coef_bytes;
                return 0;
            }
            for (int t = ch.first; t < ch.first + ch.count; t++) // (status[] of this chunk is final: its workers are done)
                if (status[take[(size_t)t]] == HVC_OK && infos[take[(size_t)t]].coef_count) ok.push_back(take[(size_t)t]);
            if (ok.empty()) return 0;
            coef_total += ch.coef_bytes;
            return ch.coef_bytes;
        },
        [&](int k, int slot) {
            if (gpu) { // the reader in front of the block stage; the chunk's good files are known from its verdict
                if (gpu_upload_err != hipSuccess) return fail_hip(c, gpu_upload_err);
                const hvc::MixedDecodeChunk &ch = chunks[(size_t)k];
                int n_gpu = 0;
                const int rc = rd.read(k, c->d_ring[slot].as<int16_t>(), c->stream, back, &n_gpu);
                if (rc) return rc;
                gpu_files += (unsigned long long)n_gpu;
                for (int t = ch.first; t < ch.first + ch.count; t++)
                    if (!back[(size_t)take[(size_t)t]] && infos[take[(size_t)t]].coef_count) ok.push_back(take[(size_t)t]);
                if (ok.empty()) return (int)HVC_OK;
            }
            const int16_t *coefs = c->d_ring[slot].as<const int16_t>();
            const int n_ok = (int)ok.size();
            uint8_t *dst = out ? out : c->d_oring[slot].as<uint8_t>();
            if (!form.rgb()) return mixed_launch(c, coefs, coef_rel.data(), oinfos, ok.data(), n_ok, dst, dst_off, c->profiling, N);
            // The planes into the slot of their own ring, the colour pass from there to where the planes would have gone.  Resized:
            // the colour pass into the slot of the RGB ring instead (tight images at decoded size), the two resampling passes from
            // there to where the images would have gone.  Every plan is built before anything is enqueued.
            const bool resized = form.resized();
            uint8_t *planes = c->d_pring[slot].as<uint8_t>(), *rgb = resized ? c->d_rring[slot].as<uint8_t>() : dst;
            hvc::MixedRgbPlan cplan;
            hvc::ResizePlan rplan;
            int rc = hvc::mixed_rgb_plan_build(oinfos, plan.plane_rel.data(), resized ? plan.rgb_rel.data() : dst_off,
                                               resized ? nullptr : form.rgb_row_strides, form.layout, ok.data(), n_ok, (uintptr_t)planes,
                                               (uintptr_t)rgb, true, cplan, N);
            if (!rc && resized) {
                hvc::ResizePlanOpts po;
                po.boxes = form.boxes, po.mirror = form.mirror, po.out_elem = form.out_elem;
                rc = hvc::resize_plan_build_opts(plan.rimg.data(), ok.data(), n_ok, form.layout, form.filter, (uintptr_t)rgb, (uintptr_t)dst, po, rplan);
            }
            if (!rc && resized && rplan.mid_bytes > c->d_mring[slot].cap) rc = HVC_E_INTERNAL;
            if (!rc) rc = mixed_launch(c, coefs, coef_rel.data(), oinfos, ok.data(), n_ok, planes, plan.plane_rel.data(), c->profiling, N);
            if (!rc) rc = mixed_rgb_launch_plan(c, cplan, form.layout, planes, rgb, false);
            if (!rc && resized) rc = resize_launch_plan(c, rplan, rgb, dst, c->d_mring[slot].as<uint8_t>(), false, form.lut);
            return rc;
        },
        [&](int k, int slot) {
            hipError_t he = hipSuccess;
            if (where != HVC_MEM_HOST) return he;
            // what the kernels wrote and nothing else: never a failed file's record, never the caller's row padding
            hvc::mixed_decode_download_runs(plan, k, status, gpu ? back.data() : nullptr, form, N != 8, host_reader_only, runs);
            uint8_t *to = pixels + chunks[(size_t)k].pix_lo;
            const uint8_t *from = c->d_oring[slot].as<const uint8_t>();
            for (const hvc::MixedDecodeRun &run : runs) {
                if (he != hipSuccess) break;
                he = run.rows ? hipMemcpy2DAsync(to + run.lo, run.row_stride, from + run.lo, run.row_stride, run.row_bytes, run.rows,
                                                 hipMemcpyDeviceToHost, c->stream)
                              : hipMemcpyAsync(to + run.lo, from + run.lo, run.bytes, hipMemcpyDeviceToHost, c->stream);
            }
            return he;
        },
        stats);
    if (stats) {
        stats->entropy_ms_sum = (double)entropy_ns.load() * 1e-6;
        stats->frames_per_chunk = plan.largest;
        stats->coef_bytes = coef_total;
    }
    if (host_reader_only) return r;
    c->mixed_gpu_files = gpu_files;
    c->mixed_host_files = (unsigned long long)n_take - gpu_files;
    if (!gpu || r != HVC_OK || gpu_files == (unsigned long long)n_take) return r;
    // The handed-back files, through this pipeline with the host reader: every other file masked out by its status.
    std::vector<int> kept((size_t)n_files);
    for (int f = 0; f < n_files; f++) {
        kept[(size_t)f] = status[f];
        if (status[f] == HVC_OK && !(chunk_of[(size_t)f] >= 0 && back[(size_t)f])) status[f] = HVC_E_INTERNAL;
    }
    hvc_batch_stats tail;
    r = decode_batch_mixed_impl(c, jpegs, sizes, n_files, threads, chunk_bytes, infos, status, pixel_offsets, pixels, pixel_cap, where, &tail,
                                form, true);
    for (int f = 0; f < n_files; f++)
        if (!(kept[(size_t)f] == HVC_OK && chunk_of[(size_t)f] >= 0 && back[(size_t)f])) status[f] = kept[(size_t)f];
    if (stats) {
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        stats->entropy_ms_sum += tail.entropy_ms_sum;
        stats->h2d_ms_sum += tail.h2d_ms_sum;
        stats->kernel_ms_sum += tail.kernel_ms_sum;
        stats->d2h_ms_sum += tail.d2h_ms_sum;
        stats->chunks += tail.chunks;
    }
    return r;
}
