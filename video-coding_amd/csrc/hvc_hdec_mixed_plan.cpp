// hvc_hdec_mixed_plan.cpp -- host plan of the mixed GPU Huffman reader (hvc_hdec_mixed_plan.h): per-file descriptors, the
// distinct table sets and the unit map of one chunk.  Plain C++ (no device code), usable without a GPU.
#include <cstring>
#include <new>

#include "hvc_hdec_mixed_plan.h"

namespace hvc {

int hdm_geometry(const hvc_jpeg_info &info, HdmFileK &k) {
    std::memset(&k, 0, sizeof k);
    if (info.n_comp < 1 || info.n_comp > 3) return HDM_NO_COMPONENTS;
    const hvc_jpeg_component &c0 = info.comp[0];
    if (c0.hscale < 1 || c0.vscale < 1) return HDM_NO_COMPONENTS;
    const long long mbs_wide = c0.decoded_width / (8 * c0.hscale), mbs_high = c0.decoded_height / (8 * c0.vscale);
    if (mbs_wide < 0 || mbs_high < 0) return HDM_TOO_LARGE;
    long long base = 0;
    for (int i = 0; i < info.n_comp; i++) {
        const long long h = info.comp[i].hscale, v = info.comp[i].vscale;
        if (h < 1 || v < 1) return HDM_NO_COMPONENTS;
        // the decoder raises when the MCU grid leaves a plane ("Plane.set out of bounds"): the host reader decides
        if (mbs_wide * h > info.layout[i].blocks_w || mbs_high * v > info.layout[i].blocks_h) return HDM_MCU_GRID;
        if (base + h * v > HVC_HD_MAX_MCU_BLOCKS) return HDM_MCU_BLOCKS;
        if (info.layout[i].coef_offset >= (1ull << 32) || (info.layout[i].coef_offset & 7)) return HDM_TOO_LARGE;
        k.h[i] = (unsigned)h;
        k.v[i] = (unsigned)v;
        k.bw[i] = (unsigned)info.layout[i].blocks_w;
        k.mcu_base[i] = (unsigned)base;
        k.coef_off[i] = (unsigned)info.layout[i].coef_offset;
        for (long long q = 0; q < h * v; q++) {
            k.b2comp[base + q] = (unsigned char)i;
            k.b2sy[base + q] = (unsigned char)(q / h);
            k.b2sx[base + q] = (unsigned char)(q % h);
            k.selmask |= (unsigned)i << (2 * (base + q));
        }
        base += h * v;
    }
    const unsigned long long bpf = (unsigned long long)mbs_wide * (unsigned long long)mbs_high * (unsigned long long)base;
    if (bpf == 0) return HDM_NO_BLOCKS;
    if (bpf >= (1ull << 31) || info.coef_count >= (1ull << 32) || mbs_wide >= (1ll << 31)) return HDM_TOO_LARGE;
    k.n_comp = (unsigned)info.n_comp;
    k.blocks_per_mcu = (unsigned)base;
    k.mbs_wide = (unsigned)mbs_wide;
    k.need = (unsigned)bpf;
    return HDM_TAKEN;
}

int hdm_plan_build(const HdmFileIn *files, int n_files, const int *list, int n_list, HdmPlan &plan) {
    plan = HdmPlan();
    if (n_list < 0 || n_files < 0 || (n_list > 0 && !files)) return HVC_E_INVALID_ARG;
    const size_t SB = HVC_HD_SUBSEQ_BITS / 8;
    try {
        plan.refusal.assign((size_t)n_list, HDM_TAKEN);
        unsigned long long subs = 0, units = 0, dcd = 0;
        for (int l = 0; l < n_list; l++) {
            const int f = list ? list[l] : l;
            if (f < 0 || f >= n_files) return HVC_E_INVALID_ARG;
            const HdmFileIn &in = files[f];
            if (!in.info || !in.tables) return HVC_E_INVALID_ARG;
            HdmFileK k;
            int why = hdm_geometry(*in.info, k);
            if (!why && !in.tables_ok) why = HDM_TABLES;
            if (!why && ((in.coef_base & 7) || (in.ecs_off % SB))) why = HDM_PLACE;
            const unsigned long long n_sub = hdm_file_subs(in.seg_bytes), n_units = (n_sub + HVC_HDM_UNIT - 1) / HVC_HDM_UNIT;
            // 32-bit indices: bit positions inside a file, subsequences and units of the chunk, bytes of the segment buffer,
            // entries of the DC rows
            if (!why && ((unsigned long long)in.seg_bytes >= (1ull << 28) || subs + n_sub >= (1ull << 31) ||
                         (unsigned long long)in.ecs_off + hdm_file_room(in.seg_bytes) >= (1ull << 32) || dcd + k.need >= (1ull << 32)))
                why = HDM_TOO_LARGE;
            plan.refusal[(size_t)l] = why;
            if (why) continue;
            k.ecs_off = (unsigned)in.ecs_off;
            k.sub0 = (unsigned)subs;
            k.n_sub = (unsigned)n_sub;
            k.unit0 = (unsigned)units;
            k.coef_base = in.coef_base;
            k.dcd0 = (unsigned)dcd;
            // its table record: newest first (files of one source tend to come in runs)
            if (in.tabrec >= 0) { // the caller's index: the record is named by the first listed file that carries it
                if ((size_t)in.tabrec >= plan.tab_src.size()) plan.tab_src.resize((size_t)in.tabrec + 1, -1);
                if (plan.tab_src[(size_t)in.tabrec] < 0) plan.tab_src[(size_t)in.tabrec] = f;
                k.tabrec = (unsigned)in.tabrec;
            } else {
                size_t t = plan.tab_src.size();
                while (t > 0 && (plan.tab_src[t - 1] < 0 || std::memcmp(files[plan.tab_src[t - 1]].tables, in.tables, sizeof(HdTables)))) t--;
                if (t == 0) {
                    plan.tab_src.push_back(f);
                    t = plan.tab_src.size();
                }
                k.tabrec = (unsigned)(t - 1);
            }
            const unsigned at = (unsigned)plan.files.size();
            plan.files.push_back(k);
            plan.file_of.push_back(f);
            plan.map.insert(plan.map.end(), (size_t)n_units, at);
            subs += n_sub;
            units += n_units;
            dcd += k.need;
            const size_t end = in.ecs_off + hdm_file_room(in.seg_bytes);
            if (end > plan.seg_bytes) plan.seg_bytes = end;
        }
        plan.total_sub = (unsigned)subs;
        plan.dcd_entries = (size_t)dcd;
    } catch (const std::bad_alloc &) {
        return HVC_E_OUT_OF_MEMORY;
    }
    return HVC_OK;
}

} // namespace hvc
