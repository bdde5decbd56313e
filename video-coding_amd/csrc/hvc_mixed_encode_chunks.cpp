// hvc_mixed_encode_chunks.cpp -- the chunk cut of the two mixed encode file pipelines and the host-only parts of their
// padding workers (hvc_mixed_encode_chunks.h).  Plain C++ (no HIP), usable without a GPU.
#include "hvc_mixed_encode_chunks.h"

#include <algorithm>
#include <cstring>

#include "hvc_mixed_encode_plan.h"
#include "hvc_mixed_rgb_plan.h"

void encode_frame_spans(const hvc_jpeg_info &fi, size_t &pixel_span, size_t &coef_span) {
    pixel_span = coef_span = 0;
    for (int i = 0; i < fi.n_comp && i < 4; i++) {
        const hvc_component &k = fi.layout[i];
        if (k.blocks_w <= 0 || k.blocks_h <= 0) continue;
        coef_span = std::max(coef_span, k.coef_offset + (size_t)k.blocks_w * k.blocks_h * 64);
        pixel_span = std::max(pixel_span, k.plane_offset + ((size_t)k.blocks_h * 8 - 1) * k.stride + (size_t)k.blocks_w * 8);
    }
}

void pad_frame(const hvc_jpeg_info &info, const uint8_t *src, uint8_t *rec) {
    for (int i = 0; i < 3; i++) {
        const hvc_component &L = info.layout[i];
        const int sw = info.comp[i].actual_width, sh = info.comp[i].actual_height;
        const int pw = info.comp[i].decoded_width, ph = info.comp[i].decoded_height;
        const int bw = sw < pw ? sw : pw, bh = sh < ph ? sh : ph;
        uint8_t *dst = rec + L.plane_offset;
        for (int row = 0; row < ph; row++) {
            uint8_t *d = dst + (size_t)row * L.stride;
            if (row < bh) {
                std::memcpy(d, src + (size_t)row * sw, (size_t)bw);
                std::memset(d + bw, 0, (size_t)(pw - bw)); // Plane.create is zero-filled
            } else {
                std::memset(d, 0, (size_t)pw);
            }
        }
        src += (size_t)sw * sh;
    }
}

int encode_rgb_frame_status(const hvc_jpeg_info &info, const MixedEncodeInput &in, int f) {
    const int s = rgb_sampling_of(info);
    if (s != HVC_YUV_420 && s != HVC_YUV_422 && s != HVC_YUV_444) return HVC_E_INVALID_ARG;
    if ((s != HVC_YUV_444 && (info.width & 1)) || (s == HVC_YUV_420 && (info.height & 1))) return HVC_E_INVALID_ARG; // Yuv.assert_is_420 / _422
    if (in.rgb_row_strides && in.rgb_row_strides[f] && in.rgb_row_strides[f] < hvc::mixed_rgb_row_bytes(in.layout, info.width)) return HVC_E_INVALID_ARG;
    return HVC_OK;
}

size_t encode_rgb_frame_bytes(const hvc_jpeg_info &info, const MixedEncodeInput &in) {
    return hvc::mixed_rgb_row_bytes(in.layout, info.width) * hvc::mixed_rgb_rows(in.layout, info.height);
}

void encode_rgb_frame_copy(const hvc_jpeg_info &info, const MixedEncodeInput &in, int f, const uint8_t *src, uint8_t *dst) {
    const size_t row = hvc::mixed_rgb_row_bytes(in.layout, info.width), rows = hvc::mixed_rgb_rows(in.layout, info.height);
    const size_t rs = in.rgb_row_strides && in.rgb_row_strides[f] ? in.rgb_row_strides[f] : row;
    if (rs == row) {
        std::memcpy(dst, src, row * rows);
        return;
    }
    for (size_t y = 0; y < rows; y++) std::memcpy(dst + y * row, src + y * rs, row); // (planar: the planes are rs * height apart)
}

namespace hvc {

int mixed_encode_chunks_build(const hvc_jpeg_info *infos, int *status, const uint8_t *const *frames, uint8_t *const *jpegs, int n_frames,
                              size_t chunk_bytes, const MixedEncodeInput &in, int max_files_per_chunk, MixedEncodeChunks &plan) {
    plan = MixedEncodeChunks();
    if (n_frames < 0 || (n_frames > 0 && (!infos || !status || !frames || !jpegs))) return HVC_E_INVALID_ARG;
    if (chunk_bytes == 0) chunk_bytes = (size_t)64 << 20;
    plan.chunk_of.assign((size_t)n_frames, -1);
    plan.pix_rel.assign((size_t)n_frames, 0);
    plan.coef_rel.assign((size_t)n_frames, 0);
    plan.rgb_rel.assign(in.rgb ? (size_t)n_frames : 0, 0);
    std::vector<MixedEncodeChunk> &chunks = plan.chunks;
    for (int f = 0; f < n_frames; f++) {
        if (status[f] != HVC_OK) continue;
        if (!frames[f] || !jpegs[f]) return HVC_E_INVALID_ARG;
        const size_t zero = 0;
        MixedEncodePlan own;
        int e = hvc_jpeg_encoder_check(&infos[f]);
        if (!e) e = mixed_encode_plan_build(&infos[f], &zero, &zero, nullptr, 1, own);
        if (!e && (infos[f].pixel_bytes == 0 || infos[f].coef_count == 0)) e = HVC_E_INVALID_ARG;
        for (int i = 0; i < 3 && !e; i++) { // what the padding workers go by
            const hvc_jpeg_component &k = infos[f].comp[i];
            if (k.decoded_width != 8 * infos[f].layout[i].blocks_w || k.decoded_height != 8 * infos[f].layout[i].blocks_h ||
                k.actual_width < 0 || k.actual_height < 0)
                e = HVC_E_INVALID_ARG;
        }
        if (!e && in.rgb) e = encode_rgb_frame_status(infos[f], in, f);
        if (e) {
            status[f] = e;
            continue;
        }
        size_t ps, cs;
        encode_frame_spans(infos[f], ps, cs);
        if (ps > infos[f].pixel_bytes || cs > infos[f].coef_count) return HVC_E_INVALID_ARG; // (not a record of the layout call)
        const size_t pb = (infos[f].pixel_bytes + 63) & ~(size_t)63;
        if (chunks.empty() || (chunks.back().count > 0 && (chunks.back().pix_bytes + pb > chunk_bytes ||
                                                           (max_files_per_chunk > 0 && chunks.back().count >= max_files_per_chunk)))) {
            chunks.emplace_back();
            chunks.back().first = (int)plan.take.size();
        }
        MixedEncodeChunk &k = chunks.back();
        plan.pix_rel[(size_t)f] = k.pix_bytes;
        plan.coef_rel[(size_t)f] = k.coef_elems;
        plan.chunk_of[(size_t)f] = (int)chunks.size() - 1;
        k.pix_bytes += pb;
        k.coef_elems += (infos[f].coef_count + 31) & ~(size_t)31;
        if (in.rgb) { // the tight image in the chunk's RGB slot, on 64 bytes
            plan.rgb_rel[(size_t)f] = k.rgb_bytes;
            k.rgb_bytes += (encode_rgb_frame_bytes(infos[f], in) + 63) & ~(size_t)63;
        }
        k.count++;
        plan.take.push_back(f);
    }
    for (const MixedEncodeChunk &k : chunks) {
        plan.in_bytes = std::max(plan.in_bytes, std::max(k.pix_bytes, k.rgb_bytes));
        plan.rgb_bytes = std::max(plan.rgb_bytes, k.rgb_bytes);
        plan.out_bytes = std::max(plan.out_bytes, k.coef_elems * sizeof(int16_t));
        plan.largest = std::max(plan.largest, k.count);
        plan.coef_total += k.coef_elems * sizeof(int16_t);
    }
    return HVC_OK;
}

} // namespace hvc
