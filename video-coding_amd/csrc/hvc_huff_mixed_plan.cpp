// hvc_huff_mixed_plan.cpp -- the host plan of the mixed GPU Huffman coder and its hand-back decision
// (hvc_huff_mixed_plan.h).  Plain C++ (no HIP), usable without a GPU.
#include "hvc_huff_mixed_plan.h"

namespace hvc {

int huff_mixed_geometry(const hvc_jpeg_info &info, bool optimised, HuffMixedFileK &k, HuffMixedPlaneK (&planes)[3]) {
    const int r = hvc_jpeg_encoder_check(&info); // (n_comp != 3 among the rest)
    if (r) return r;
    k = HuffMixedFileK();
    const hvc_jpeg_component &c0 = info.comp[0];
    k.mbs_wide = c0.decoded_width / (8 * c0.hscale);
    k.mbs_high = c0.decoded_height / (8 * c0.vscale);
    int base = 0;
    for (int i = 0; i < 3; i++) {
        HuffMixedPlaneK &p = planes[i];
        p = HuffMixedPlaneK();
        const hvc_component &l = info.layout[i];
        if (l.blocks_w <= 0 || l.blocks_h <= 0) return HVC_E_INVALID_ARG;
        if ((long long)l.blocks_w * l.blocks_h > 0x7fffffffll - HVC_MIXED_UNIT) return HVC_E_TOO_LARGE;
        if (l.coef_offset & 7) return HVC_E_ALIGNMENT;
        p.bw = l.blocks_w;
        p.nblk = l.blocks_w * l.blocks_h;
        p.h = info.comp[i].hscale;
        p.v = info.comp[i].vscale;
        p.mcu_base = base;
        p.table = info.comp[i].dc_table ? 1 : 0;
        p.coef_base = l.coef_offset;
        base += p.h * p.v;
    }
    k.blocks_per_mcu = base;
    // a table set that no component selects has no symbol to fit a table to (hvc_huffman_optimal_tables refuses it too)
    if (optimised && planes[0].table == planes[1].table && planes[1].table == planes[2].table) return HVC_E_INVALID_ARG;
    if (k.mbs_wide <= 0 || k.mbs_high <= 0 || base <= 0) return HVC_E_INVALID_ARG; // no coded block
    const unsigned long long bpf = (unsigned long long)k.mbs_wide * (unsigned long long)k.mbs_high * (unsigned long long)base;
    if (bpf * 64ull * 27ull >= (1ull << 32)) return HVC_E_TOO_LARGE; // 32-bit bit offsets per file (huffman_prepare's bound)
    k.blocks = (unsigned)bpf;
    // worst case per block: 64 fields of 27 bits (216 bytes), as huffman_prepare sizes a frame's buffer
    const unsigned long long words = (bpf * 216 + 3) / 4 + 2;
    k.bitbuf_words = (unsigned)((words + 15) / 16 * 16);
    return HVC_OK;
}

int huff_mixed_plan_build(const hvc_jpeg_info *infos, const size_t *coef_offsets, const int *frames, int n_list, bool optimised,
                          HuffMixedPlan &plan) {
    plan = HuffMixedPlan();
    if (n_list < 0 || (n_list > 0 && (!infos || !coef_offsets))) return HVC_E_INVALID_ARG;
    for (int t = 0; frames && t < n_list; t++)
        if (frames[t] < 0) return HVC_E_INVALID_ARG;
    plan.status.assign((size_t)n_list, HVC_OK);
    unsigned long long units = 0;
    for (int t = 0; t < n_list; t++) {
        const int f = frames ? frames[t] : t;
        HuffMixedFileK k;
        HuffMixedPlaneK p[3];
        int r = huff_mixed_geometry(infos[f], optimised, k, p);
        if (!r && (coef_offsets[f] & 7)) r = HVC_E_ALIGNMENT;
        if (r) {
            plan.status[(size_t)t] = r;
            continue;
        }
        k.lens_base = plan.lens_total;
        k.bitbuf_base = plan.bitbuf_words;
        plan.lens_total += k.blocks;
        plan.bitbuf_words += k.bitbuf_words;
        for (int i = 0; i < 3; i++) {
            p[i].coef_base += coef_offsets[f];
            p[i].unit0 = (unsigned)units;
            p[i].file = (unsigned)plan.files.size();
            const unsigned n_units = ((unsigned)p[i].nblk + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT;
            units += n_units;
            if (units > HVC_MIXED_MAX_UNITS) {
                plan = HuffMixedPlan();
                return HVC_E_TOO_LARGE;
            }
            plan.map.insert(plan.map.end(), n_units, (unsigned)plan.planes.size());
            plan.planes.push_back(p[i]);
        }
        plan.coef_elems += infos[f].coef_count;
        plan.files.push_back(k);
        plan.file_of.push_back(f);
    }
    plan.pieces_cap = plan.bitbuf_words / 16;
    if (plan.files.size() > HVC_HUFF_MIXED_MAX_FILES || plan.pieces_cap >= (1ull << 32) || plan.lens_total >= (1ull << 32)) {
        plan = HuffMixedPlan();
        return HVC_E_TOO_LARGE;
    }
    return HVC_OK;
}

void huff_mixed_hand_back(const unsigned long long *offsets, const unsigned *file_status, int n_files, unsigned long long capacity,
                          std::vector<int> &complete, std::vector<int> &handed_back) {
    complete.clear();
    handed_back.clear();
    bool past = false;
    for (int k = 0; k < n_files; k++) {
        if (offsets[k + 1] > capacity) past = true; // (offsets never decrease: every later file ends past it too)
        if (past || file_status[k])
            handed_back.push_back(k);
        else
            complete.push_back(k);
    }
}

} // namespace hvc
