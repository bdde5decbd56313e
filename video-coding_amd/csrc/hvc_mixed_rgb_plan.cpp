// hvc_mixed_rgb_plan.cpp -- host plan of the colour pass over a mixed batch: mixed_rgb_layout behind
// hvc_jpeg_mixed_rgb_layout (where every file's RGB image goes) and the descriptor builder behind hvc_yuv_to_rgb_mixed /
// hvc_decode_frames_mixed_rgb / hvc_jpeg_decode_batch_mixed_rgb (hvc_mixed_rgb_plan.h); with them the two rules every RGB
// entry point reads a file's sampling and chroma window by.  Plain C++ (no HIP), usable without a GPU.
#include <cstring>
#include <new>

#include "hvc_mixed_rgb_plan.h"

int rgb_sampling_of(const hvc_jpeg_info &info) {
    if (info.n_comp == 1) return HVC_YUV_400;
    if (info.n_comp != 3) return 0;
    const hvc_jpeg_component *k = info.comp;
    if (k[1].hscale != k[2].hscale || k[1].vscale != k[2].vscale || k[1].hscale < 1 || k[1].vscale < 1) return 0;
    if (k[0].hscale == k[1].hscale && k[0].vscale == k[1].vscale) return HVC_YUV_444;
    if (k[0].hscale == 2 * k[1].hscale && k[0].vscale == 2 * k[1].vscale) return HVC_YUV_420;
    if (k[0].hscale == 2 * k[1].hscale && k[0].vscale == k[1].vscale) return HVC_YUV_422;
    return 0;
}

void rgb_chroma_window(int sampling, int width, int height, int &cw, int &ch) {
    cw = sampling == HVC_YUV_444 ? width : (width + 1) / 2;
    ch = sampling == HVC_YUV_420 ? (height + 1) / 2 : height;
}

namespace hvc {

int mixed_rgb_plan_build(const hvc_jpeg_info *infos, const size_t *yuv_offsets, const size_t *rgb_offsets, const size_t *rgb_row_strides,
                         int layout, const int *frames, int n_list, uintptr_t yuv_addr, uintptr_t rgb_addr, bool decoded,
                         MixedRgbPlan &plan, int n) {
    plan.images.clear();
    plan.map.clear();
    plan.frame.clear();
    plan.lanes = 0;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (n != 8 && n != 4 && n != 2 && n != 1) return HVC_E_INVALID_ARG;
    if (n_list < 0 || (n_list > 0 && (!infos || !yuv_offsets || !rgb_offsets))) return HVC_E_INVALID_ARG;
    unsigned long long units = 0;
    for (int l = 0; l < n_list; l++) {
        const int f = frames ? frames[l] : l;
        if (f < 0) return HVC_E_INVALID_ARG;
        const hvc_jpeg_info &fi = infos[f];
        if (fi.width < 0 || fi.height < 0) return HVC_E_INVALID_ARG;
        if (fi.width == 0 || fi.height == 0) continue; // no pixel: no descriptor, no unit
        const int sampling = rgb_sampling_of(fi);
        if (!sampling) return HVC_E_INVALID_ARG;
        if (fi.width > (1 << 24) || fi.height > (1 << 24)) return HVC_E_TOO_LARGE;
        const bool grey = sampling == HVC_YUV_400;
        MixedRgbImageK k;
        std::memset(&k, 0, sizeof k);
        k.w = fi.width, k.h = fi.height, k.sampling = sampling;
        if (!grey) rgb_chroma_window(sampling, k.w, k.h, k.cw, k.ch);
        for (int i = 0; i < (grey ? 1 : 3); i++) { // rows long enough and, where the component names its blocks, the window inside them
            const hvc_component &c = fi.layout[i];
            const int pw = i ? k.cw : k.w, ph = i ? k.ch : k.h;
            if (c.stride < (size_t)pw) return HVC_E_INVALID_ARG;
            if (c.blocks_w < 0 || c.blocks_h < 0 || (decoded && (c.blocks_w == 0 || c.blocks_h == 0))) return HVC_E_INVALID_ARG;
            if (c.blocks_w > 0 && c.blocks_h > 0 && (pw > n * (long long)c.blocks_w || ph > n * (long long)c.blocks_h)) return HVC_E_INVALID_ARG;
            const unsigned long long base = (unsigned long long)yuv_offsets[f] + c.plane_offset;
            (i == 0 ? k.y_base : i == 1 ? k.cb_base : k.cr_base) = base;
            (i == 0 ? k.y_stride : i == 1 ? k.cb_stride : k.cr_stride) = c.stride;
        }
        const size_t tight = mixed_rgb_row_bytes(layout, k.w);
        k.row_stride = rgb_row_strides && rgb_row_strides[f] ? rgb_row_strides[f] : tight;
        if (k.row_stride < tight) return HVC_E_INVALID_ARG;
        k.plane_stride = k.row_stride * (unsigned long long)k.h;
        k.rgb_base = rgb_offsets[f];
        k.groups = ((unsigned)k.w + 7) >> 3;
        const unsigned long long lrows = sampling == HVC_YUV_420 ? ((unsigned)k.h + 1) >> 1 : (unsigned)k.h;
        const unsigned long long lanes = k.groups * lrows;
        // lane row = umulhi(t, magic) is exact for t * groups < 2^32 (magic = (2^32 + e) / groups, e < groups)
        if (lanes * k.groups >= (1ull << 32) || lanes >= (1ull << 31)) return HVC_E_TOO_LARGE;
        k.lanes = (unsigned)lanes;
        k.magic = k.groups == 1 ? 0u : (unsigned)(((1ull << 32) + k.groups - 1) / k.groups);
        const unsigned long long nu = (lanes + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT;
        if (units + nu > HVC_MIXED_MAX_UNITS) return HVC_E_TOO_LARGE;
        k.unit0 = (unsigned)units;
        // the 8-byte (chroma of 4:2:0 / 4:2:2: 4-byte) forms: every row of the plane / image starts on that boundary
        const unsigned long long ca = sampling == HVC_YUV_444 ? 8 : 4;
        k.vec_y = (((unsigned long long)yuv_addr + k.y_base) | k.y_stride) % 8 == 0;
        k.vec_c = !grey && (((unsigned long long)yuv_addr + k.cb_base) | ((unsigned long long)yuv_addr + k.cr_base) | k.cb_stride | k.cr_stride) % ca == 0;
        k.vec_rgb = (((unsigned long long)rgb_addr + k.rgb_base) | k.row_stride | (layout == HVC_RGB_PLANAR ? k.plane_stride : 0)) % 8 == 0;
        plan.images.push_back(k);
        plan.frame.push_back(f);
        units += nu;
        plan.lanes += lanes;
    }
    plan.map.reserve((size_t)units); // (filled once the whole set is accepted: a refused set costs no memory)
    for (size_t i = 0; i < plan.images.size(); i++)
        plan.map.insert(plan.map.end(), ((size_t)plan.images[i].lanes + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT, (unsigned)i);
    return HVC_OK;
}

// The encode direction (k_rgb_to_ycc_mixed): the same tables, with the lane count of k_rgb_to_ycc -- h / 2 lane rows for
// 4:2:0, chroma rows of w / 2 -- and the encoder's even-size rule in place of the decode direction's ceil windows.
int mixed_rgb_encode_plan_build(const hvc_jpeg_info *infos, const size_t *yuv_offsets, const size_t *rgb_offsets,
                                const size_t *rgb_row_strides, int layout, const int *frames, int n_list, uintptr_t yuv_addr,
                                uintptr_t rgb_addr, MixedRgbPlan &plan) {
    plan.images.clear();
    plan.map.clear();
    plan.frame.clear();
    plan.lanes = 0;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (n_list < 0 || (n_list > 0 && (!infos || !yuv_offsets || !rgb_offsets))) return HVC_E_INVALID_ARG;
    unsigned long long units = 0;
    for (int l = 0; l < n_list; l++) {
        const int f = frames ? frames[l] : l;
        if (f < 0) return HVC_E_INVALID_ARG;
        const hvc_jpeg_info &fi = infos[f];
        if (fi.width < 0 || fi.height < 0) return HVC_E_INVALID_ARG;
        const int sampling = rgb_sampling_of(fi);
        if (sampling != HVC_YUV_420 && sampling != HVC_YUV_422 && sampling != HVC_YUV_444) return HVC_E_INVALID_ARG;
        // Yuv.assert_is_420 / _422: what hvc_rgb_to_yuv and hvc_jpeg_encode_rgb refuse
        if (sampling != HVC_YUV_444 && (fi.width & 1)) return HVC_E_INVALID_ARG;
        if (sampling == HVC_YUV_420 && (fi.height & 1)) return HVC_E_INVALID_ARG;
        if (fi.width == 0 || fi.height == 0) continue; // no pixel: no descriptor, no unit
        if (fi.width > (1 << 24) || fi.height > (1 << 24)) return HVC_E_TOO_LARGE;
        MixedRgbImageK k;
        std::memset(&k, 0, sizeof k);
        k.w = fi.width, k.h = fi.height, k.sampling = sampling;
        k.cw = sampling == HVC_YUV_444 ? k.w : k.w / 2;
        k.ch = sampling == HVC_YUV_420 ? k.h / 2 : k.h;
        for (int i = 0; i < 3; i++) { // rows long enough and, where the component names its blocks, the samples inside them
            const hvc_component &c = fi.layout[i];
            const int pw = i ? k.cw : k.w, ph = i ? k.ch : k.h;
            if (c.stride < (size_t)pw) return HVC_E_INVALID_ARG;
            if (c.blocks_w < 0 || c.blocks_h < 0) return HVC_E_INVALID_ARG;
            if (c.blocks_w > 0 && c.blocks_h > 0 && (pw > 8 * (long long)c.blocks_w || ph > 8 * (long long)c.blocks_h)) return HVC_E_INVALID_ARG;
            const unsigned long long base = (unsigned long long)yuv_offsets[f] + c.plane_offset;
            (i == 0 ? k.y_base : i == 1 ? k.cb_base : k.cr_base) = base;
            (i == 0 ? k.y_stride : i == 1 ? k.cb_stride : k.cr_stride) = c.stride;
        }
        const size_t tight = mixed_rgb_row_bytes(layout, k.w);
        k.row_stride = rgb_row_strides && rgb_row_strides[f] ? rgb_row_strides[f] : tight;
        if (k.row_stride < tight) return HVC_E_INVALID_ARG;
        k.plane_stride = k.row_stride * (unsigned long long)k.h;
        k.rgb_base = rgb_offsets[f];
        k.groups = ((unsigned)k.w + 7) >> 3;
        const unsigned long long lrows = sampling == HVC_YUV_420 ? (unsigned)k.h >> 1 : (unsigned)k.h;
        const unsigned long long lanes = k.groups * lrows;
        if (lanes * k.groups >= (1ull << 32) || lanes >= (1ull << 31)) return HVC_E_TOO_LARGE; // (as mixed_rgb_plan_build)
        k.lanes = (unsigned)lanes;
        k.magic = k.groups == 1 ? 0u : (unsigned)(((1ull << 32) + k.groups - 1) / k.groups);
        const unsigned long long nu = (lanes + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT;
        if (units + nu > HVC_MIXED_MAX_UNITS) return HVC_E_TOO_LARGE;
        k.unit0 = (unsigned)units;
        const unsigned long long ca = sampling == HVC_YUV_444 ? 8 : 4;
        k.vec_y = (((unsigned long long)yuv_addr + k.y_base) | k.y_stride) % 8 == 0;
        k.vec_c = (((unsigned long long)yuv_addr + k.cb_base) | ((unsigned long long)yuv_addr + k.cr_base) | k.cb_stride | k.cr_stride) % ca == 0;
        k.vec_rgb = (((unsigned long long)rgb_addr + k.rgb_base) | k.row_stride | (layout == HVC_RGB_PLANAR ? k.plane_stride : 0)) % 8 == 0;
        plan.images.push_back(k);
        plan.frame.push_back(f);
        units += nu;
        plan.lanes += lanes;
    }
    plan.map.reserve((size_t)units);
    for (size_t i = 0; i < plan.images.size(); i++)
        plan.map.insert(plan.map.end(), ((size_t)plan.images[i].lanes + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT, (unsigned)i);
    return HVC_OK;
}

// hvc_jpeg_encoder_mixed_rgb_layout (include/hvc_jpeg.h; the entry point itself stands in hvc_capi_files.hip)
int encoder_mixed_rgb_layout(const int *widths, const int *heights, const int *chromas, const int *qualities, int n_frames, int layout,
                             size_t align, size_t row_align, hvc_jpeg_info *infos, int *status, size_t *rgb_offsets,
                             size_t *rgb_row_strides, size_t *rgb_total, size_t *pixel_offsets, size_t *coef_offsets, size_t *pixel_total,
                             size_t *coef_total) {
    if (!widths || !heights || !chromas || !qualities || !infos || !status || !rgb_offsets || !rgb_row_strides || !rgb_total ||
        !pixel_offsets || !coef_offsets || !pixel_total || !coef_total || n_frames < 0)
        return HVC_E_INVALID_ARG;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (align == 0) align = 256;
    if (row_align == 0) row_align = 1;
    if ((align & (align - 1)) || (row_align & (row_align - 1))) return HVC_E_INVALID_ARG;
    size_t rend = 0, pend = 0, cend = 0; // the ends of the last records placed
    for (int f = 0; f < n_frames; f++) {
        const int w = widths[f], h = heights[f], s = chromas[f];
        status[f] = hvc_jpeg_encoder_layout(w, h, s, qualities[f], &infos[f]);
        if (status[f] == HVC_OK) status[f] = hvc_jpeg_encoder_check(&infos[f]);
        if (status[f] == HVC_OK && (((s == 420 || s == 422) && (w & 1)) || (s == 420 && (h & 1)))) status[f] = HVC_E_INVALID_ARG;
        const size_t rstart = (rend + align - 1) & ~(align - 1);
        const size_t pstart = (pend + 63) & ~(size_t)63, cstart = (cend + 7) & ~(size_t)7; // as hvc_jpeg_encoder_mixed_layout, align 0
        rgb_offsets[f] = rstart;
        rgb_row_strides[f] = 0;
        pixel_offsets[f] = pstart;
        coef_offsets[f] = cstart;
        if (status[f] != HVC_OK) continue; // takes no room
        const size_t row = (mixed_rgb_row_bytes(layout, w) + row_align - 1) & ~(row_align - 1);
        rgb_row_strides[f] = row;
        rend = rstart + row * mixed_rgb_rows(layout, h);
        pend = pstart + infos[f].pixel_bytes;
        cend = cstart + infos[f].coef_count;
    }
    *rgb_total = rend;
    *pixel_total = pend;
    *coef_total = cend;
    return HVC_OK;
}

// hvc_jpeg_mixed_rgb_layout (include/hvc_jpeg.h; the entry point itself stands in hvc_capi_jpeg.hip)
int mixed_rgb_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int layout, size_t align, size_t row_align,
                     hvc_jpeg_info *infos, int *status, size_t *rgb_offsets, size_t *rgb_row_strides, size_t *total_bytes) {
    if (!jpegs || !sizes || !infos || !status || !rgb_offsets || !rgb_row_strides || !total_bytes || n_files < 0) return HVC_E_INVALID_ARG;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (align == 0) align = 256;
    if (row_align == 0) row_align = 1;
    if ((align & (align - 1)) || (row_align & (row_align - 1))) return HVC_E_INVALID_ARG;
    size_t end = 0; // the end of the last record placed
    for (int f = 0; f < n_files; f++) {
        status[f] = jpegs[f] ? hvc_jpeg_read_header(jpegs[f], sizes[f], &infos[f]) : HVC_E_INVALID_ARG;
        if (status[f] == HVC_OK && !rgb_sampling_of(infos[f])) status[f] = HVC_E_INVALID_ARG; // as hvc_jpeg_decode_rgb answers it
        const size_t start = (end + align - 1) & ~(align - 1);
        rgb_offsets[f] = start;
        rgb_row_strides[f] = 0;
        if (status[f] != HVC_OK) continue; // takes no room
        const size_t row = (mixed_rgb_row_bytes(layout, infos[f].width) + row_align - 1) & ~(row_align - 1);
        rgb_row_strides[f] = row;
        const size_t bytes = row * mixed_rgb_rows(layout, infos[f].height);
        if (bytes == 0) continue;
        end = start + bytes;
    }
    *total_bytes = end;
    return HVC_OK;
}

// hvc_jpeg_mixed_scaled_rgb_layout (include/hvc_jpeg.h): scale_denom = 1 is mixed_rgb_layout itself, with scaled[f] == infos[f]
int mixed_scaled_rgb_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int scale_denom, int layout, size_t align,
                            size_t row_align, hvc_jpeg_info *infos, hvc_jpeg_info *scaled, int *status, size_t *rgb_offsets,
                            size_t *rgb_row_strides, size_t *total_bytes) {
    const int n = scaled_side(scale_denom);
    if (!n || !scaled) return HVC_E_INVALID_ARG;
    if (n == 8) {
        const int r = mixed_rgb_layout(jpegs, sizes, n_files, layout, align, row_align, infos, status, rgb_offsets, rgb_row_strides, total_bytes);
        for (int f = 0; !r && f < n_files; f++)
            if (status[f] == HVC_OK) scaled[f] = infos[f];
        return r;
    }
    if (!jpegs || !sizes || !infos || !status || !rgb_offsets || !rgb_row_strides || !total_bytes || n_files < 0) return HVC_E_INVALID_ARG;
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (align == 0) align = 256;
    if (row_align == 0) row_align = 1;
    if ((align & (align - 1)) || (row_align & (row_align - 1))) return HVC_E_INVALID_ARG;
    size_t end = 0; // the end of the last record placed
    for (int f = 0; f < n_files; f++) {
        status[f] = jpegs[f] ? hvc_jpeg_read_header(jpegs[f], sizes[f], &infos[f]) : HVC_E_INVALID_ARG;
        if (status[f] == HVC_OK && !rgb_sampling_of(infos[f])) status[f] = HVC_E_INVALID_ARG; // as hvc_jpeg_decode_scaled_rgb answers it
        const size_t start = (end + align - 1) & ~(align - 1);
        rgb_offsets[f] = start;
        rgb_row_strides[f] = 0;
        if (status[f] != HVC_OK) continue; // takes no room
        scaled_info(infos[f], n, scaled[f]);
        const size_t row = (mixed_rgb_row_bytes(layout, scaled[f].width) + row_align - 1) & ~(row_align - 1);
        rgb_row_strides[f] = row;
        const size_t bytes = row * mixed_rgb_rows(layout, scaled[f].height);
        if (bytes == 0) continue;
        end = start + bytes;
    }
    *total_bytes = end;
    return HVC_OK;
}

} // namespace hvc
