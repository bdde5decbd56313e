// hvc_capi_mixed_encode.hip -- ENCODING batches of frames that share neither geometry, sampling nor quality: what stands
// behind hvc_encode_frames_mixed (the forward block stage over a set of frames, one launch of k_encode_mixed,
// hvc_mixed_encode.hip) and hvc_jpeg_encode_batch_mixed (raw frames in, JPEG files out); the entry points themselves stand
// in hvc_capi_files.hip, with hvc_jpeg_encoder_mixed_layout (host only).  The host plan is hvc_mixed_encode_plan.cpp's, its
// tables go to device memory as the mixed decode plans do (upload_image).
// The file pipeline is hvc_jpeg_encode_batch's with chunks cut by bytes and a status per file:
//   host threads: Plane.blit_available into zero-padded planes (pinned ring)       encoder.ml:514-516
//   copy stream:  hipMemcpyAsync H2D           compute stream: k_encode_mixed (a plan per chunk), D2H of the chunk's records
//   host threads: write_headers + rle + write_bits + EOI per file, with its own info      encoder.ml:127-193, 371-418
// With RGB images as input (MixedEncodeInput, hvc_mixed_encode_chunks.h; behind hvc_jpeg_encode_batch_mixed_rgb) the host
// threads copy each image's rows tight into the pinned ring, the copy stream uploads them into a device RGB slot, and on the
// compute stream a hipMemsetAsync of the chunk's plane slot and k_rgb_to_ycc_mixed (hvc_mixed_rgb.hip) stand in front of
// k_encode_mixed.  The colour pass alone is behind hvc_rgb_to_yuv_mixed, in front of one block stage behind
// hvc_encode_frames_mixed_rgb (below).
// Everything up to the coefficient slot -- the chunk cut (hvc_mixed_encode_chunks.cpp, plain C++), the padding workers, the two
// chunk feeds (hvc_feed.h), upload and block stage per chunk, the way out -- is encode_mixed_chunks (MixedEncodeFront,
// hvc_batch.h), which the pipeline with the GPU coder (hvc_capi_mixed_coder.hip) runs too; encode_batch_mixed_impl adds the
// download of the records and the coder workers.
#include "hvc_batch.h"
#include "hvc_mixed_encode.h"
#include "hvc_mixed_rgb.h"

namespace {

// the plan as one image: planes | tables | map, each part on 16 bytes, in c->mixed_enc_plan
int upload_encode_plan(hvc_ctx *c, const hvc::MixedEncodePlan &plan, hvc::MixedEncodeParams &P) {
    size_t at[3];
    const int r = upload_parts(c, c->mixed_enc_plan, {{plan.planes.data(), plan.planes.size() * sizeof(hvc::MixedPlaneK)},
                                                      {plan.tables.data(), plan.tables.size() * sizeof(hvc::MixedEncTableK)},
                                                      {plan.map.data(), plan.map.size() * sizeof(unsigned)}}, at);
    if (r) return r;
    const unsigned char *d = c->mixed_enc_plan.d.as<const unsigned char>();
    P.planes = reinterpret_cast<const hvc::MixedPlaneK *>(d);
    P.tables = reinterpret_cast<const hvc::MixedEncTableK *>(d + at[1]);
    P.map = reinterpret_cast<const unsigned *>(d + at[2]);
    P.n_units = (unsigned)plan.map.size();
    return HVC_OK;
}

} // namespace

// The block stage of a plan on DEVICE memory, enqueued on c->stream
int encode_mixed_launch_plan(hvc_ctx *c, const hvc::MixedEncodePlan &plan, const uint8_t *d_pixels, int16_t *d_coefs, bool profile,
                             const MixedLibjpeg *lje) {
    if (plan.map.empty()) return HVC_OK; // no block at all: nothing to launch
    if (((uintptr_t)d_coefs & 15) || ((uintptr_t)d_pixels & 7)) return HVC_E_ALIGNMENT;
    if (lje) { // the image: planes | multiplier records | map | dummy pairs -- the last two parts only under the setting
        std::vector<hvc::FdctIslowTableK> tables;
        std::vector<hvc::DummyPairK> pairs;
        hvc::libjpeg_mixed_tables_build(plan.qt, tables);
        int r = hvc::libjpeg_mixed_dummies_build(lje->infos, lje->coef_offsets, lje->frames, lje->n_list, pairs);
        if (r) return r;
        size_t at[4];
        if ((r = upload_parts(c, c->mixed_enc_plan, {{plan.planes.data(), plan.planes.size() * sizeof(hvc::MixedPlaneK)},
                                                     {tables.data(), tables.size() * sizeof(hvc::FdctIslowTableK)},
                                                     {plan.map.data(), plan.map.size() * sizeof(unsigned)},
                                                     {pairs.data(), pairs.size() * sizeof(hvc::DummyPairK)}}, at)))
            return r;
        const unsigned char *d = c->mixed_enc_plan.d.as<const unsigned char>();
        hvc::FdctIslowMixedParams J;
        std::memset(&J, 0, sizeof J);
        J.planes = reinterpret_cast<const hvc::MixedPlaneK *>(d);
        J.tables = reinterpret_cast<const hvc::FdctIslowTableK *>(d + at[1]);
        J.map = reinterpret_cast<const unsigned *>(d + at[2]);
        J.n_units = (unsigned)plan.map.size();
        J.pixels = d_pixels;
        J.coefs = d_coefs;
        HIPCHK(c, profiled_launch(c, profile, [&](hipEvent_t k0, hipEvent_t k1) { return hvc::launch_fdct_islow_mixed(J, c->stream, k0, k1); }));
        HIPCHK(c, hvc::launch_dummy_blocks_mixed(d_coefs, reinterpret_cast<const hvc::DummyPairK *>(d + at[3]), (unsigned)pairs.size(), c->stream));
        return HVC_OK;
    }
    hvc::MixedEncodeParams P;
    std::memset(&P, 0, sizeof P);
    const int r = upload_encode_plan(c, plan, P);
    if (r) return r;
    P.pixels = d_pixels;
    P.coefs = d_coefs;
    HIPCHK(c, profiled_launch(c, profile, [&](hipEvent_t k0, hipEvent_t k1) { return hvc::launch_encode_mixed(P, c->stream, k0, k1); }));
    return HVC_OK;
}

// behind hvc_encode_frames_mixed (hvc_capi_files.hip)
int encode_frames_mixed_impl(hvc_ctx *c, const uint8_t *pixels, const size_t *pixel_offsets, const hvc_jpeg_info *infos, int n_frames,
                             int16_t *coefs, const size_t *coef_offsets, int where) {
    if (!c || n_frames < 0 || (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE)) return HVC_E_INVALID_ARG;
    if (c->enc_arith != HVC_ARITH_MODEL) return HVC_E_INVALID_ARG; // (the RTL encoder's arithmetic has no mixed form)
    if (n_frames == 0) return HVC_OK;
    if (!infos || !coef_offsets || !pixel_offsets) return HVC_E_INVALID_ARG;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    int r;
    hvc::MixedEncodePlan plan; // the caller's own offsets: checked for either kind of memory, launched on for device memory
    if ((r = hvc::mixed_encode_plan_build(infos, coef_offsets, pixel_offsets, nullptr, n_frames, plan))) return r;
    if (plan.map.empty()) return HVC_OK; // (a set without a block needs no memory)
    if (!coefs || !pixels) return HVC_E_INVALID_ARG;
    const MixedLibjpeg own{infos, coef_offsets, nullptr, n_frames};
    if (where == HVC_MEM_DEVICE) return encode_mixed_launch_plan(c, plan, pixels, coefs, c->profiling, c->enc_libjpeg ? &own : nullptr);
    // host memory: the frames' records one after another in c->d_in / c->d_out, each on 64 bytes; only the coefficient
    // planes come back (gaps in the caller's buffer stay untouched)
    std::vector<size_t> d_pix((size_t)n_frames, 0), d_coef((size_t)n_frames, 0), pspan((size_t)n_frames, 0);
    size_t ptot = 0, ctot = 0;
    for (int f = 0; f < n_frames; f++) {
        size_t cs;
        encode_frame_spans(infos[f], pspan[(size_t)f], cs);
        d_pix[(size_t)f] = ptot;
        d_coef[(size_t)f] = ctot;
        ptot += (pspan[(size_t)f] + 63) & ~(size_t)63;
        ctot += (cs + 31) & ~(size_t)31;
    }
    if ((r = grow(c, c->d_in, ptot))) return r;
    if ((r = grow(c, c->d_out, ctot * sizeof(int16_t)))) return r;
    if ((r = hvc::mixed_encode_plan_build(infos, d_coef.data(), d_pix.data(), nullptr, n_frames, plan))) return r;
    for (int f = 0; f < n_frames; f++)
        if (pspan[(size_t)f])
            HIPCHK(c, hipMemcpyAsync(c->d_in.as<uint8_t>() + d_pix[(size_t)f], pixels + pixel_offsets[f], pspan[(size_t)f],
                                     hipMemcpyHostToDevice, c->stream));
    const MixedLibjpeg staged{infos, d_coef.data(), nullptr, n_frames};
    if ((r = encode_mixed_launch_plan(c, plan, c->d_in.as<const uint8_t>(), c->d_out.as<int16_t>(), false, c->enc_libjpeg ? &staged : nullptr))) {
        (void)hipStreamSynchronize(c->stream);
        return r;
    }
    for (int f = 0; f < n_frames; f++)
        for (int i = 0; i < infos[f].n_comp; i++) {
            const hvc_component &k = infos[f].layout[i];
            const size_t n = (size_t)k.blocks_w * k.blocks_h * 64;
            HIPCHK(c, hipMemcpyAsync(coefs + coef_offsets[f] + k.coef_offset, c->d_out.as<const int16_t>() + d_coef[(size_t)f] + k.coef_offset,
                                     n * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
        }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HVC_OK;
}

// ---------------------------------------------------------------------------
// RGB input: k_rgb_to_ycc_mixed (hvc_mixed_rgb.hip) from the host plan mixed_rgb_encode_plan_build (hvc_mixed_rgb_plan.cpp)

namespace {

// bytes from the start of frame f's image to its last byte, by the caller's row stride (0: no image, or a stride below the row)
size_t rgb_image_span(const hvc_jpeg_info &fi, const size_t *rgb_row_strides, int f, int layout) {
    if (fi.width < 1 || fi.height < 1) return 0;
    const size_t tight = hvc::mixed_rgb_row_bytes(layout, fi.width);
    const size_t rs = rgb_row_strides && rgb_row_strides[f] ? rgb_row_strides[f] : tight;
    return rs < tight ? 0 : hvc::mixed_rgb_span(layout, fi.width, fi.height, rs);
}

} // namespace

int rgb_to_ycc_mixed_launch(hvc_ctx *c, hvc::MixedRgbPlan &plan, int layout, uint8_t *d_planes, const uint8_t *d_rgb, bool profile, bool pad,
                            const hvc_jpeg_info *infos) {
    if (!c->enc_libjpeg) return mixed_rgb_launch_plan(c, plan, layout, d_planes, const_cast<uint8_t *>(d_rgb), profile, true); // (d_rgb is read only)
    if (plan.images.empty()) return HVC_OK;
    int r = hvc::libjpeg_rgb_plan_lanes(plan, pad, infos);
    if (r) return r;
    size_t at[2];
    if ((r = upload_parts(c, c->mixed_rgb_plan, {{plan.images.data(), plan.images.size() * sizeof(hvc::MixedRgbImageK)},
                                                 {plan.map.data(), plan.map.size() * sizeof(unsigned)}}, at)))
        return r;
    hvc::RgbLibjpegMixedParams P;
    std::memset(&P, 0, sizeof P);
    P.rgb = d_rgb;
    P.yuv = d_planes;
    P.images = c->mixed_rgb_plan.d.as<const hvc::MixedRgbImageK>();
    P.map = reinterpret_cast<const unsigned *>(c->mixed_rgb_plan.d.as<const unsigned char>() + at[1]);
    P.n_units = (unsigned)plan.map.size();
    P.planar = layout == HVC_RGB_PLANAR;
    P.pad = pad;
    HIPCHK(c, profiled_launch(c, profile, [&](hipEvent_t k0, hipEvent_t k1) { return hvc::launch_rgb_to_ycc_libjpeg_mixed(P, c->stream, k0, k1); }));
    return HVC_OK;
}

namespace {

// a chunk's colour stage on c->stream: the plane slot cleared, then k_rgb_to_ycc_mixed over the listed frames
int encode_rgb_stage(hvc_ctx *c, const MixedEncodeInput &in, const hvc_jpeg_info *infos, const int *list, int count, const size_t *pix_rel,
                     const size_t *rgb_rel, const uint8_t *d_rgb, uint8_t *d_planes, size_t plane_bytes) {
    hvc::MixedRgbPlan plan;
    const int r = hvc::mixed_rgb_encode_plan_build(infos, pix_rel, rgb_rel, nullptr, in.layout, list, count, (uintptr_t)d_planes, (uintptr_t)d_rgb, plan);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(d_planes, 0, plane_bytes, c->stream)); // Plane.create is zero-filled: the kernel writes the frames' own samples only
    return rgb_to_ycc_mixed_launch(c, plan, in.layout, d_planes, d_rgb, false, true, infos); // (hvc_set_encode_libjpeg: with the replicated edge)
}

} // namespace

// behind hvc_rgb_to_yuv_mixed (hvc_yuv.hip)
int rgb_to_yuv_mixed_impl(hvc_ctx *c, uint8_t *yuv, const size_t *yuv_offsets, const hvc_jpeg_info *infos, int n_frames, const uint8_t *rgb,
                          const size_t *rgb_offsets, const size_t *rgb_row_strides, int layout, int where) {
    if (!c || n_frames < 0 || (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE)) return HVC_E_INVALID_ARG;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (n_frames == 0) return HVC_OK;
    if (!infos || !yuv_offsets || !rgb_offsets) return HVC_E_INVALID_ARG;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    int r;
    hvc::MixedRgbPlan plan; // the caller's own offsets: checked for either kind of memory, launched on for device memory
    if ((r = hvc::mixed_rgb_encode_plan_build(infos, yuv_offsets, rgb_offsets, rgb_row_strides, layout, nullptr, n_frames, (uintptr_t)yuv,
                                              (uintptr_t)rgb, plan)))
        return r;
    if (plan.map.empty()) return HVC_OK; // (a set without a pixel needs no memory)
    if (!yuv || !rgb) return HVC_E_INVALID_ARG;
    if (where == HVC_MEM_DEVICE) return rgb_to_ycc_mixed_launch(c, plan, layout, yuv, rgb, c->profiling, false, infos);
    // host memory: the images and the plane records one after another in c->d_in / c->d_out; only each frame's own samples
    // come back (the padding of its planes stays the caller's)
    std::vector<size_t> yspan((size_t)n_frames, 0), rspan((size_t)n_frames, 0), d_yuv, d_rgb;
    for (size_t i = 0; i < plan.images.size(); i++) {
        const hvc::MixedRgbImageK &k = plan.images[i];
        const int f = plan.frame[i];
        yspan[(size_t)f] = rgb_yuv_span(infos[f].layout, k.sampling, k.w, k.h, k.cw, k.ch);
        rspan[(size_t)f] = rgb_image_span(infos[f], rgb_row_strides, f, layout);
    }
    const size_t ytot = stage_offsets(yuv_offsets, yspan, d_yuv), rtot = stage_offsets(rgb_offsets, rspan, d_rgb);
    if ((r = grow(c, c->d_in, rtot))) return r;
    if ((r = grow(c, c->d_out, ytot))) return r;
    if ((r = hvc::mixed_rgb_encode_plan_build(infos, d_yuv.data(), d_rgb.data(), rgb_row_strides, layout, nullptr, n_frames, (uintptr_t)c->d_out.p,
                                              (uintptr_t)c->d_in.p, plan)))
        return r;
    for (int f = 0; f < n_frames; f++)
        if (rspan[(size_t)f])
            HIPCHK(c, hipMemcpyAsync(c->d_in.as<uint8_t>() + d_rgb[(size_t)f], rgb + rgb_offsets[f], rspan[(size_t)f], hipMemcpyHostToDevice, c->stream));
    if ((r = rgb_to_ycc_mixed_launch(c, plan, layout, c->d_out.as<uint8_t>(), c->d_in.as<const uint8_t>(), false, false, infos))) {
        (void)hipStreamSynchronize(c->stream);
        return r;
    }
    for (size_t i = 0; i < plan.images.size(); i++) {
        const hvc::MixedRgbImageK &k = plan.images[i];
        const int f = plan.frame[i];
        for (int p = 0; p < 3; p++) {
            const hvc_component &L = infos[f].layout[p];
            const size_t at = L.plane_offset;
            HIPCHK(c, hipMemcpy2DAsync(yuv + yuv_offsets[f] + at, L.stride, c->d_out.as<const uint8_t>() + d_yuv[(size_t)f] + at, L.stride,
                                       (size_t)(p ? k.cw : k.w), (size_t)(p ? k.ch : k.h), hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HVC_OK;
}

// behind hvc_encode_frames_mixed_rgb (hvc_capi_files.hip): zeroed padded planes in c->d_aux (tight records on 64 bytes), the
// colour pass into them, k_encode_mixed from there; host memory: the images are staged in c->d_in, the records in c->d_out
int encode_frames_mixed_rgb_impl(hvc_ctx *c, const uint8_t *rgb, const size_t *rgb_offsets, const size_t *rgb_row_strides, int layout,
                                 const hvc_jpeg_info *infos, int n_frames, int16_t *coefs, const size_t *coef_offsets, int where) {
    if (!c || n_frames < 0 || (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE)) return HVC_E_INVALID_ARG;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (c->enc_arith != HVC_ARITH_MODEL) return HVC_E_INVALID_ARG; // (the RTL encoder's arithmetic has no mixed form)
    if (n_frames == 0) return HVC_OK;
    if (!infos || !coef_offsets || !rgb_offsets) return HVC_E_INVALID_ARG;
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    const bool host = where == HVC_MEM_HOST;
    std::vector<size_t> d_pix((size_t)n_frames, 0), d_coef((size_t)n_frames, 0), rspan((size_t)n_frames, 0), d_rgb;
    size_t ptot = 0, ctot = 0;
    for (int f = 0; f < n_frames; f++) {
        size_t ps, cs;
        encode_frame_spans(infos[f], ps, cs);
        d_pix[(size_t)f] = ptot;
        d_coef[(size_t)f] = ctot;
        ptot += (ps + 63) & ~(size_t)63;
        ctot += (cs + 31) & ~(size_t)31;
        rspan[(size_t)f] = rgb_image_span(infos[f], rgb_row_strides, f, layout);
    }
    const size_t rtot = host ? stage_offsets(rgb_offsets, rspan, d_rgb) : 0;
    int r;
    hvc::MixedEncodePlan bplan; // both plans before anything is enqueued: a set that is refused leaves nothing behind
    hvc::MixedRgbPlan cplan;
    if ((r = hvc::mixed_encode_plan_build(infos, host ? d_coef.data() : coef_offsets, d_pix.data(), nullptr, n_frames, bplan))) return r;
    if ((r = hvc::mixed_rgb_encode_plan_build(infos, d_pix.data(), host ? d_rgb.data() : rgb_offsets, rgb_row_strides, layout, nullptr, n_frames, 0,
                                              host ? 0 : (uintptr_t)rgb, cplan)))
        return r;
    if (bplan.map.empty()) return HVC_OK; // (a set without a block needs no memory)
    if (!coefs || (!cplan.map.empty() && !rgb)) return HVC_E_INVALID_ARG;
    if (!host && ((uintptr_t)coefs & 15)) return HVC_E_ALIGNMENT;
    if ((r = grow(c, c->d_aux, ptot))) return r;
    if (host && (r = grow(c, c->d_in, rtot))) return r;
    if (host && (r = grow(c, c->d_out, ctot * sizeof(int16_t)))) return r;
    const uint8_t *src = host ? c->d_in.as<const uint8_t>() : rgb;
    // (the flags follow the actual addresses: the plan again, now that the scratch is there)
    if ((r = hvc::mixed_rgb_encode_plan_build(infos, d_pix.data(), host ? d_rgb.data() : rgb_offsets, rgb_row_strides, layout, nullptr, n_frames,
                                              (uintptr_t)c->d_aux.p, (uintptr_t)src, cplan)))
        return r;
    for (int f = 0; host && f < n_frames; f++)
        if (rspan[(size_t)f])
            HIPCHK(c, hipMemcpyAsync(c->d_in.as<uint8_t>() + d_rgb[(size_t)f], rgb + rgb_offsets[f], rspan[(size_t)f], hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_aux.p, 0, ptot, c->stream)); // Plane.create is zero-filled
    r = rgb_to_ycc_mixed_launch(c, cplan, layout, c->d_aux.as<uint8_t>(), src, false, true, infos);
    const MixedLibjpeg lje{infos, host ? d_coef.data() : coef_offsets, nullptr, n_frames};
    if (!r) r = encode_mixed_launch_plan(c, bplan, c->d_aux.as<const uint8_t>(), host ? c->d_out.as<int16_t>() : coefs, !host && c->profiling,
                                         c->enc_libjpeg ? &lje : nullptr);
    if (r) {
        (void)hipStreamSynchronize(c->stream);
        return r;
    }
    if (!host) return HVC_OK;
    for (int f = 0; f < n_frames; f++)
        for (int i = 0; i < infos[f].n_comp; i++) {
            const hvc_component &k = infos[f].layout[i];
            const size_t n = (size_t)k.blocks_w * k.blocks_h * 64;
            HIPCHK(c, hipMemcpyAsync(coefs + coef_offsets[f] + k.coef_offset, c->d_out.as<const int16_t>() + d_coef[(size_t)f] + k.coef_offset,
                                     n * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
        }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HVC_OK;
}

// ---------------------------------------------------------------------------
// The file pipelines: what both run (MixedEncodeFront, hvc_batch.h), then the one with the host coder

int encode_mixed_chunks(hvc_ctx *c, const uint8_t *const *frames, const hvc_jpeg_info *infos, int *status, int n_frames, int threads,
                        size_t chunk_bytes, uint8_t *const *jpegs, const MixedEncodeInput &in, MixedEncodeFront &fr, hvc_batch_stats *stats) {
    if (threads < 1) threads = 1;
    if (threads > 256) threads = 256;
    constexpr int NB = hvc_ctx::RING;
    // the frames that take part, cut into chunks by the bytes of their padded pixel records; a frame the block stage or the
    // coder would refuse gets its own status here and is left out
    const hvc::MixedEncodeChunks &plan = fr.plan;
    int r = hvc::mixed_encode_chunks_build(infos, status, frames, jpegs, n_frames, chunk_bytes, in, fr.max_files_per_chunk, fr.plan);
    if (r || plan.take.empty()) return r;
    const int n_chunks = (int)plan.chunks.size(), n_take = (int)plan.take.size();

    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    HIPCHK(c, c->copy_stream.ensure());
    if (fr.down_stream) HIPCHK(c, c->down_stream.ensure());
    for (int i = 0; i < NB; i++) {
        HIPCHK(c, c->ev_up[i].ensure());
        HIPCHK(c, c->ev_down[i].ensure());
        for (int k = 0; k < 3; k++) HIPCHK(c, c->ev_et[i][k].ensure());
        if (fr.down_stream) HIPCHK(c, c->ev_gpu[i].ensure());
    }
    // (a frame larger than chunk_bytes: the ring grows)
    if ((r = ring_ensure(c, enc_rings(c), {plan.in_bytes, plan.out_bytes, plan.in_bytes, plan.out_bytes}))) return r;
    if (in.rgb && (r = ring_ensure(c, enc_rgb_rings(c), {plan.rgb_bytes}))) return r;
    if (fr.setup && (r = fr.setup())) return r;

    std::atomic<long long> pad_ns{0};
    fr.wall0 = std::chrono::steady_clock::now();
    fr.threads = threads;
    const int pad_threads = (threads + 3) / 4; // (padding is a copy: a quarter of the coder's threads keeps ahead of them)
    if ((r = pool_ready(c, threads, pad_threads))) return r;
    fr.ran = true;
    bool left = false; // the coder feed goes first when the call is left: it ends the padding workers with it
    hvc::ChunkFeed padf(c->pool, n_chunks, NB);
    // ring 0: chunk k may be read by the pipeline's workers once release(k) says what they read has landed
    hvc::ChunkFeed codf(c->pool, n_chunks, 0, [&] { if (!left) padf.raise(HVC_E_INTERNAL); });
    fr.codf = &codf;
    auto pad_worker = [&]() {
        if (!pin_to_ctx_cpus(c)) padf.raise(HVC_E_INVALID_ARG); // hvc_set_host_cpus
        for (;;) {
            const int t = padf.claim();
            if (t >= n_take || padf.error()) return;
            const int f = plan.take[(size_t)t], k = plan.chunk_of[(size_t)f];
            if (!padf.wait_slot(k)) return;
            const auto t0 = std::chrono::steady_clock::now();
            if (in.rgb)
                encode_rgb_frame_copy(infos[f], in, f, frames[f], c->eh_in[k % NB].as<uint8_t>() + plan.rgb_rel[(size_t)f]);
            else
                (c->enc_libjpeg ? hvc::pad_frame_replicate : pad_frame)(infos[f], frames[f], c->eh_in[k % NB].as<uint8_t>() + plan.pix_rel[(size_t)f]);
            pad_ns += MixedEncodeFront::ns_since(t0);
            padf.report(k, 1, HVC_OK);
        }
    };
    r = padf.start(pad_threads, pad_worker);
    if (!r) r = codf.start(threads, fr.worker);

    int rc = r;
    hipStream_t compute = c->stream;
    try {
        for (int k = 0; k < n_chunks && rc == HVC_OK; k++) {
            const hvc::MixedEncodeChunk &ch = plan.chunks[(size_t)k];
            const int slot = k % NB;
            const int *list = plan.take.data() + ch.first;
            if ((rc = padf.wait_chunk(k, ch.count))) break;
            // what the slot holds behind the block stage is free again once chunk k - NB has left the pipeline's workers (its
            // downloads and the kernels that read the device slots are behind it: ev_down[slot] was waited for before that
            // chunk went to them)
            if (k >= NB && (rc = codf.wait_chunk(k - NB, plan.chunks[(size_t)(k - NB)].count))) break;
            hipError_t he = hipEventRecord(c->ev_et[slot][0], c->copy_stream);
            if (he == hipSuccess)
                he = in.rgb ? hipMemcpyAsync(c->ed_rgb[slot].p, c->eh_in[slot].p, ch.rgb_bytes, hipMemcpyHostToDevice, c->copy_stream)
                            : hipMemcpyAsync(c->ed_in[slot].p, c->eh_in[slot].p, ch.pix_bytes, hipMemcpyHostToDevice, c->copy_stream);
            if (he == hipSuccess) he = hipEventRecord(c->ev_up[slot], c->copy_stream);
            if (he == hipSuccess) he = hipStreamWaitEvent(compute, c->ev_up[slot], 0);
            if (he == hipSuccess) he = hipEventRecord(c->ev_et[slot][1], compute);
            if (he != hipSuccess) { rc = fail_hip(c, he); break; }
            if (in.rgb && (rc = encode_rgb_stage(c, in, infos, list, ch.count, plan.pix_rel.data(), plan.rgb_rel.data(),
                                                 c->ed_rgb[slot].as<const uint8_t>(), c->ed_in[slot].as<uint8_t>(), ch.pix_bytes)))
                break;
            hvc::MixedEncodePlan bplan;
            if ((rc = hvc::mixed_encode_plan_build(infos, plan.coef_rel.data(), plan.pix_rel.data(), list, ch.count, bplan))) break;
            const MixedLibjpeg lje{infos, plan.coef_rel.data(), list, ch.count};
            if ((rc = encode_mixed_launch_plan(c, bplan, c->ed_in[slot].as<const uint8_t>(), c->ed_out[slot].as<int16_t>(), false,
                                               c->enc_libjpeg ? &lje : nullptr)))
                break;
            if ((rc = fr.stage(k, slot))) break;
            // wait for this chunk's upload, then hand the pinned pixel slot to chunk k + NB
            he = wait_event(c->ev_up[slot]);
            if (he != hipSuccess) { rc = fail_hip(c, he); break; }
            padf.release(k);
            if ((rc = fr.retire(k))) break; // (while this chunk's kernels run)
        }
        if (rc == HVC_OK) rc = fr.drain();
        for (int k = std::max(0, n_chunks - NB); k < n_chunks && rc == HVC_OK; k++) rc = codf.wait_chunk(k, plan.chunks[(size_t)k].count);
    } catch (...) {
        rc = hvc::exception_code();
    }
    if (rc != HVC_OK) { // both feeds end before either waits for the pool
        padf.raise(rc);
        codf.raise(rc);
    }
    left = true;
    rc = padf.finish(rc);
    rc = codf.finish(rc);
    fr.codf = nullptr;
    {
        const hipError_t h1 = hipStreamSynchronize(compute), h2 = hipStreamSynchronize(c->copy_stream),
                         h3 = fr.down_stream ? hipStreamSynchronize(c->down_stream) : hipSuccess;
        if (rc == HVC_OK && (h1 != hipSuccess || h2 != hipSuccess || h3 != hipSuccess))
            rc = fail_hip(c, h1 != hipSuccess ? h1 : h2 != hipSuccess ? h2 : h3);
    }
    if (stats) {
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - fr.wall0).count();
        stats->host_prep_ms_sum = (double)pad_ns.load() * 1e-6;
        stats->h2d_ms_sum = fr.h2d_ms;
        stats->kernel_ms_sum = fr.k_ms;
        stats->d2h_ms_sum = fr.d2h_ms;
        stats->chunks = n_chunks;
        stats->threads = threads;
        stats->frames_per_chunk = plan.largest;
    }
    return rc;
}

// behind hvc_jpeg_encode_batch_mixed (hvc_capi_files.hip)
int encode_batch_mixed_impl(hvc_ctx *c, const uint8_t *const *frames, const hvc_jpeg_info *infos, int *status, int n_frames, int threads,
                            size_t chunk_bytes, uint8_t *const *jpegs, const size_t *caps, size_t *sizes, hvc_batch_stats *stats,
                            const MixedEncodeInput &in) {
    if (!c || !frames || !infos || !status || !jpegs || !caps || !sizes || n_frames < 0) return HVC_E_INVALID_ARG;
    if (c->enc_arith != HVC_ARITH_MODEL) return HVC_E_INVALID_ARG;
    if (in.rgb && in.layout != HVC_RGB_INTERLEAVED && in.layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_frames == 0) return HVC_OK;
    constexpr int NB = hvc_ctx::RING;
    const bool opt = c->huff_tables == HVC_HUFF_OPTIMISED; // each file its own tables (hvc_set_huffman_tables)
    const int ri = c->restart_interval;                    // DRI + RSTn every ri MCUs (hvc_set_restart_interval)
    std::atomic<long long> ent_ns{0};
    MixedEncodeFront fr;
    const hvc::MixedEncodeChunks &plan = fr.plan;
    fr.worker = [&]() {
        hvc::ChunkFeed &codf = *fr.codf;
        if (!pin_to_ctx_cpus(c)) codf.raise(HVC_E_INVALID_ARG);
        for (;;) {
            const int t = codf.claim();
            if (t >= (int)plan.take.size() || codf.error()) return;
            const int f = plan.take[(size_t)t], k = plan.chunk_of[(size_t)f];
            if (!codf.wait_slot(k)) return;
            const auto t0 = std::chrono::steady_clock::now();
            const int16_t *cf = c->eh_out[k % NB].as<const int16_t>() + plan.coef_rel[(size_t)f];
            const int e = opt ? hvc::entropy_encode_optimised(&infos[f], cf, jpegs[f], caps[f], &sizes[f], ri)
                              : hvc::entropy_encode_file(&infos[f], nullptr, cf, jpegs[f], caps[f], &sizes[f], ri);
            ent_ns += MixedEncodeFront::ns_since(t0);
            status[f] = e; // the file's own result: it stops nobody else
            codf.report(k, 1, HVC_OK);
        }
    };
    // behind the block stage: the chunk's records come down on the compute stream
    fr.stage = [&](int k, int slot) {
        hipError_t he = hipEventRecord(c->ev_et[slot][2], c->stream);
        if (he == hipSuccess)
            he = hipMemcpyAsync(c->eh_out[slot].p, c->ed_out[slot].p, plan.chunks[(size_t)k].coef_elems * sizeof(int16_t), hipMemcpyDeviceToHost,
                                c->stream);
        if (he == hipSuccess) he = hipEventRecord(c->ev_down[slot], c->stream);
        return he == hipSuccess ? (int)HVC_OK : fail_hip(c, he);
    };
    // chunk j's records have landed: its times are read, its pinned slot goes to the coder workers
    auto landed = [&](int j) {
        const int slot = j % NB;
        const hipError_t he = wait_event(c->ev_down[slot]);
        if (he != hipSuccess) return fail_hip(c, he);
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev_et[slot][0], c->ev_up[slot]) == hipSuccess) fr.h2d_ms += ms;
        if (hipEventElapsedTime(&ms, c->ev_et[slot][1], c->ev_et[slot][2]) == hipSuccess) fr.k_ms += ms;
        if (hipEventElapsedTime(&ms, c->ev_et[slot][2], c->ev_down[slot]) == hipSuccess) fr.d2h_ms += ms;
        fr.codf->release(j);
        return (int)HVC_OK;
    };
    fr.retire = [&](int k) { return k > 0 ? landed(k - 1) : (int)HVC_OK; };
    fr.drain = [&]() { return landed((int)plan.chunks.size() - 1); };
    const int rc = encode_mixed_chunks(c, frames, infos, status, n_frames, threads, chunk_bytes, jpegs, in, fr, stats);
    if (stats && fr.ran) {
        stats->entropy_ms_sum = (double)ent_ns.load() * 1e-6;
        stats->coef_bytes = plan.coef_total; // bytes downloaded
    }
    return rc;
}
