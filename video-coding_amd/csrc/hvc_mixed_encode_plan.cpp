// hvc_mixed_encode_plan.cpp -- host plan of a mixed encode batch: encoder_mixed_layout behind hvc_jpeg_encoder_mixed_layout
// (where every frame's padded pixel record and coefficient record go) and the descriptor builder behind
// hvc_encode_frames_mixed / hvc_jpeg_encode_batch_mixed (hvc_mixed_encode_plan.h).  Plain C++ (no HIP), usable without a GPU.
#include "hvc_mixed_encode_plan.h"

namespace hvc {

int mixed_encode_plan_build(const hvc_jpeg_info *infos, const size_t *coef_offsets, const size_t *pixel_offsets, const int *frames,
                            int n_list, MixedEncodePlan &plan) {
    plan.planes.clear();
    plan.tables.clear();
    plan.qt.clear();
    plan.map.clear();
    plan.blocks = 0;
    if (n_list < 0 || (n_list > 0 && (!infos || !coef_offsets || !pixel_offsets))) return HVC_E_INVALID_ARG;
    for (int l = 0; l < n_list; l++) { // the encoding entry points refuse the model's empty plane (hvc_component)
        const int f = frames ? frames[l] : l;
        if (f < 0) return HVC_E_INVALID_ARG;
        const hvc_jpeg_info &fi = infos[f];
        if (fi.n_comp < 0 || fi.n_comp > 4) return HVC_E_INVALID_ARG;
        for (int i = 0; i < fi.n_comp; i++)
            if (fi.layout[i].blocks_w == 0 || fi.layout[i].blocks_h == 0) return HVC_E_INVALID_ARG;
    }
    MixedPlan d; // planes, units and map are the decode plan's; its table entries name the distinct tables
    const int r = mixed_plan_build(infos, coef_offsets, pixel_offsets, frames, n_list, d);
    if (r) return r;
    plan.tables.resize(d.tables.size());
    plan.qt.resize(d.tables.size() * 64);
    for (size_t k = 0; k < d.tables.size(); k++)
        for (int i = 0; i < 64; i++) {
            const int t = d.tables[k].qt[i];
            if (t < 1 || t > 255) { // (Markers.Dqt element_precision = 8; a zero does not divide)
                plan.tables.clear();
                plan.qt.clear();
                return HVC_E_RANGE;
            }
            plan.tables[k].qrcp[i] = encode_quant_reciprocal((unsigned)t);
            plan.qt[k * 64 + (size_t)i] = t;
        }
    plan.planes.swap(d.planes);
    plan.map.swap(d.map);
    plan.blocks = d.blocks;
    return HVC_OK;
}

int encoder_mixed_layout(const int *widths, const int *heights, const int *chromas, const int *qualities, int n_frames, size_t align,
                         hvc_jpeg_info *infos, int *status, size_t *pixel_offsets, size_t *coef_offsets, size_t *pixel_total,
                         size_t *coef_total) {
    if (!widths || !heights || !chromas || !qualities || !infos || !status || !pixel_offsets || !coef_offsets || !pixel_total ||
        !coef_total || n_frames < 0)
        return HVC_E_INVALID_ARG;
    if (align == 0) align = 64;
    if (align < 8 || (align & (align - 1))) return HVC_E_INVALID_ARG;
    size_t pend = 0, cend = 0; // the ends of the last records placed
    for (int f = 0; f < n_frames; f++) {
        status[f] = hvc_jpeg_encoder_layout(widths[f], heights[f], chromas[f], qualities[f], &infos[f]);
        if (status[f] == HVC_OK) status[f] = hvc_jpeg_encoder_check(&infos[f]);
        const size_t pstart = (pend + align - 1) & ~(align - 1), cstart = (cend + 7) & ~(size_t)7; // (int16 elements: 16 bytes)
        pixel_offsets[f] = pstart;
        coef_offsets[f] = cstart;
        if (status[f] != HVC_OK) continue; // takes no room
        pend = pstart + infos[f].pixel_bytes;
        cend = cstart + infos[f].coef_count;
    }
    *pixel_total = pend;
    *coef_total = cend;
    return HVC_OK;
}

} // namespace hvc
