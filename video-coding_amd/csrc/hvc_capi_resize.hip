// hvc_capi_resize.hip -- the resampling step over a mixed set behind hvc_rgb_resize_mixed / _opts, and the launch of a plan's two
// passes that the file pipeline ends in (hvc_jpeg_decode_batch_mixed_resized / _opts: decode_batch_mixed_impl, hvc_capi_mixed.hip).
// The host plan is hvc_resize_plan.cpp, the kernels k_resize_h_mixed / k_resize_v_mixed / k_resize_v_mixed_lut (hvc_resize.hip).
#include "hvc_batch.h"
#include "hvc_resize.h"

// The two passes of a plan on DEVICE memory, enqueued on c->stream: the plan's tables (horizontal descriptors | map | vertical
// descriptors | map | records | taps, each part on 16 bytes) go to c->resize_plan, a buffer of their own.  d_mid: at least
// plan.mid_bytes, on 64 bytes.  A pass without a unit launches nothing.  profile: the pair of the profiling ring brackets both.
// A plan made for a typed output (plan.out_elem 2 / 4): lut = the caller's table in HOST memory, 3 * 256 elements, which travels
// behind the taps, and the vertical pass is k_resize_v_mixed_lut.
int resize_launch_plan(hvc_ctx *c, const hvc::ResizePlan &plan, const uint8_t *d_src, uint8_t *d_dst, uint8_t *d_mid, bool profile,
                       const void *lut) {
    if (plan.h.map.empty() && plan.v.map.empty()) return HVC_OK;
    if (plan.out_elem && !lut) return HVC_E_INVALID_ARG;
    const size_t lut_bytes = plan.out_elem ? (size_t)3 * 256 * (size_t)plan.out_elem : 0;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    size_t at[8];
    at[0] = 0;
    at[1] = at[0] + up(plan.h.images.size() * sizeof(hvc::ResizeImageK));
    at[2] = at[1] + up(plan.h.map.size() * sizeof(unsigned));
    at[3] = at[2] + up(plan.v.images.size() * sizeof(hvc::ResizeImageK));
    at[4] = at[3] + up(plan.v.map.size() * sizeof(unsigned));
    at[5] = at[4] + up(plan.recs.size() * sizeof(hvc::ResizeRecK));
    at[6] = at[5] + up(plan.taps.size() * sizeof(int));
    at[7] = at[6] + up(lut_bytes);
    std::vector<unsigned char> img(at[7], 0);
    auto put = [&](size_t where, const void *p, size_t n) {
        if (n) std::memcpy(img.data() + where, p, n);
    };
    put(at[0], plan.h.images.data(), plan.h.images.size() * sizeof(hvc::ResizeImageK));
    put(at[1], plan.h.map.data(), plan.h.map.size() * sizeof(unsigned));
    put(at[2], plan.v.images.data(), plan.v.images.size() * sizeof(hvc::ResizeImageK));
    put(at[3], plan.v.map.data(), plan.v.map.size() * sizeof(unsigned));
    put(at[4], plan.recs.data(), plan.recs.size() * sizeof(hvc::ResizeRecK));
    put(at[5], plan.taps.data(), plan.taps.size() * sizeof(int));
    put(at[6], lut, lut_bytes);
    const int r = upload_image(c, c->resize_plan, img);
    if (r) return r;
    const unsigned char *d = c->resize_plan.d.as<const unsigned char>();
    hvc::ResizeParams P;
    std::memset(&P, 0, sizeof P);
    P.src[0] = d_src, P.src[1] = d_mid;
    P.dst[0] = d_dst, P.dst[1] = d_mid;
    P.recs = reinterpret_cast<const hvc::ResizeRecK *>(d + at[4]);
    P.taps = reinterpret_cast<const int *>(d + at[5]);
    // (one entry of the profiling ring around the two passes)
    HIPCHK(c, profiled_launch(c, profile, [&](hipEvent_t k0, hipEvent_t k1) {
               hipError_t e = k0 ? hipEventRecord(k0, c->stream) : hipSuccess;
               if (e != hipSuccess) return e;
               P.images = reinterpret_cast<const hvc::ResizeImageK *>(d + at[0]);
               P.map = reinterpret_cast<const unsigned *>(d + at[1]);
               P.n_units = (unsigned)plan.h.map.size();
               if ((e = hvc::launch_resize_h_mixed(P, c->stream)) != hipSuccess) return e;
               P.images = reinterpret_cast<const hvc::ResizeImageK *>(d + at[2]);
               P.map = reinterpret_cast<const unsigned *>(d + at[3]);
               P.n_units = (unsigned)plan.v.map.size();
               e = plan.out_elem ? hvc::launch_resize_v_mixed_lut(P, d + at[6], plan.out_elem, c->stream) : hvc::launch_resize_v_mixed(P, c->stream);
               if (e != hipSuccess) return e;
               return k1 ? hipEventRecord(k1, c->stream) : hipSuccess;
           }));
    return HVC_OK;
}

// behind hvc_rgb_resize_mixed and hvc_rgb_resize_mixed_opts (hvc_yuv.hip); opts NULL or all zero: the call without them
int rgb_resize_mixed_impl(hvc_ctx *c, const uint8_t *src, const size_t *src_offsets, const size_t *src_row_strides, const int *widths,
                          const int *heights, int n_images, uint8_t *dst, const size_t *dst_offsets, const size_t *dst_row_strides,
                          const int *out_widths, const int *out_heights, int layout, int filter, int where, const hvc_resize_opts *opts) {
    if (!c || n_images < 0 || (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE)) return HVC_E_INVALID_ARG;
    if (resize_opts_check(opts)) return HVC_E_INVALID_ARG;
    hvc::ResizePlanOpts po;
    if (opts) po.boxes = opts->boxes, po.mirror = opts->mirror, po.out_elem = opts->out_elem;
    const void *lut = opts ? opts->lut : nullptr;
    const size_t elem = po.out_elem ? (size_t)po.out_elem : 1;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (filter != HVC_RESIZE_BOX && filter != HVC_RESIZE_BILINEAR && filter != HVC_RESIZE_BICUBIC) return HVC_E_INVALID_ARG;
    if (n_images == 0) return HVC_OK;
    if (!src || !dst || !src_offsets || !dst_offsets || !widths || !heights || !out_widths || !out_heights) return HVC_E_INVALID_ARG;
    std::vector<hvc::ResizeImage> images((size_t)n_images);
    for (int i = 0; i < n_images; i++) {
        hvc::ResizeImage &im = images[(size_t)i];
        im.w = widths[i], im.h = heights[i], im.out_w = out_widths[i], im.out_h = out_heights[i];
        im.src_offset = src_offsets[i], im.src_row_stride = src_row_strides ? src_row_strides[i] : 0;
        im.dst_offset = dst_offsets[i], im.dst_row_stride = dst_row_strides ? dst_row_strides[i] : 0;
    }
    DeviceGuard g(c->device);
    if (!g.ok) return fail_hip(c, hipErrorInvalidDevice);
    hvc::ResizePlan plan; // the caller's own offsets: checked for either kind of memory, launched on for device memory
    int r = hvc::resize_plan_build_opts(images.data(), nullptr, n_images, layout, filter, (uintptr_t)src, (uintptr_t)dst, po, plan);
    if (r) return r;
    if (where == HVC_MEM_DEVICE) {
        if ((r = grow(c, c->d_aux, std::max<size_t>(plan.mid_bytes, 64)))) return r;
        return resize_launch_plan(c, plan, src, dst, c->d_aux.as<uint8_t>(), c->profiling, lut);
    }
    // host memory: the images and their outputs one after another in c->d_in / c->d_out, each keeping its offset modulo 64
    std::vector<size_t> sspan((size_t)n_images), dspan((size_t)n_images), d_src, d_dst;
    for (int i = 0; i < n_images; i++) {
        const hvc::ResizeImage &im = images[(size_t)i];
        sspan[(size_t)i] = hvc::resize_span(layout, im.w, im.h, im.src_row_stride ? im.src_row_stride : hvc::resize_row_bytes(layout, im.w));
        const size_t drow = hvc::resize_row_bytes(layout, im.out_w) * elem; // (a typed row: elem bytes per sample)
        dspan[(size_t)i] = (hvc::resize_rows(layout, im.out_h) - 1) * (im.dst_row_stride ? im.dst_row_stride : drow) + drow;
    }
    const size_t stot = stage_offsets(src_offsets, sspan, d_src), dtot = stage_offsets(dst_offsets, dspan, d_dst);
    if ((r = grow(c, c->d_in, stot))) return r;
    if ((r = grow(c, c->d_out, dtot))) return r;
    std::vector<hvc::ResizeImage> staged = images;
    for (int i = 0; i < n_images; i++) staged[(size_t)i].src_offset = d_src[(size_t)i], staged[(size_t)i].dst_offset = d_dst[(size_t)i];
    if ((r = hvc::resize_plan_build_opts(staged.data(), nullptr, n_images, layout, filter, (uintptr_t)c->d_in.p, (uintptr_t)c->d_out.p, po, plan))) return r;
    if ((r = grow(c, c->d_aux, std::max<size_t>(plan.mid_bytes, 64)))) return r;
    for (int i = 0; i < n_images; i++)
        HIPCHK(c, hipMemcpyAsync(c->d_in.as<uint8_t>() + d_src[(size_t)i], src + src_offsets[i], sspan[(size_t)i], hipMemcpyHostToDevice, c->stream));
    if ((r = resize_launch_plan(c, plan, c->d_in.as<const uint8_t>(), c->d_out.as<uint8_t>(), c->d_aux.as<uint8_t>(), false, lut))) {
        (void)hipStreamSynchronize(c->stream);
        return r;
    }
    for (int i = 0; i < n_images; i++) { // only the rows written
        const hvc::ResizeImage &im = images[(size_t)i];
        const size_t row = hvc::resize_row_bytes(layout, im.out_w) * elem, rows = hvc::resize_rows(layout, im.out_h);
        const size_t rs = im.dst_row_stride ? im.dst_row_stride : row;
        const uint8_t *from = c->d_out.as<const uint8_t>() + d_dst[(size_t)i];
        uint8_t *to = dst + dst_offsets[i];
        if (rs == row)
            HIPCHK(c, hipMemcpyAsync(to, from, row * rows, hipMemcpyDeviceToHost, c->stream));
        else
            HIPCHK(c, hipMemcpy2DAsync(to, rs, from, rs, row, rows, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HVC_OK;
}
