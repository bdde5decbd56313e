// hvc_mixed_plan.cpp -- host plan of a mixed batch: mixed_layout / mixed_scaled_layout behind hvc_jpeg_mixed_layout / hvc_jpeg_mixed_scaled_layout
// (where every file's pixel record goes) and the
// descriptor builder behind hvc_decode_frames_mixed / hvc_jpeg_decode_batch_mixed (hvc_mixed_plan.h).  Plain C++ (no HIP),
// usable without a GPU.
#include <cstring>
#include <new>

#include "hvc_idct_spec.h"
#include "hvc_mixed_plan.h"

namespace hvc {
namespace {

// jpeg/model/src/zigzag.ml:71-137  forward[raster] = zz
const unsigned char ZF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                              41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                              46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// the kernel-side forms of one table (what prepare_tables of hvc_capi.hip makes for the kernarg segment)
void table_entry(const uint16_t *q, MixedTableK &t) {
    std::memset(&t, 0, sizeof t);
    unsigned qmax = 1;
    for (int i = 0; i < 64; i++) {
        t.qt[i] = (int)q[i];
        if (q[i] > qmax) qmax = q[i];
    }
    const unsigned long long m = HVC_GUARD_D_PACKED / qmax, thr = m * m;
    t.ethr_packed = thr > 0x7ffffffeull ? 0x7ffffffe : (int)thr;
    t.wide = qmax > 255;
    static const int PAIRS[4][2] = {{HVC_PAIR_A_LO, HVC_PAIR_A_HI}, {HVC_PAIR_B_LO, HVC_PAIR_B_HI},
                                    {HVC_PAIR_C_LO, HVC_PAIR_C_HI}, {HVC_PAIR_Z_LO, HVC_PAIR_Z_HI}};
    for (int r = 0; r < 8; r++)
        for (int k = 0; k < 4; k++) {
            const unsigned lo = q[ZF[8 * r + PAIRS[k][0]]], hi = q[ZF[8 * r + PAIRS[k][1]]];
            t.qpair[r * 4 + k] = (lo & 0xffffu) | (hi << 16);
        }
}

} // namespace

int mixed_plan_build(const hvc_jpeg_info *infos, const size_t *coef_offsets, const size_t *pixel_offsets, const int *frames,
                     int n_list, MixedPlan &plan, int n, uintptr_t pix_addr) {
    plan.planes.clear();
    plan.tables.clear();
    plan.map.clear();
    plan.blocks = 0;
    if (n != 8 && n != 4 && n != 2 && n != 1) return HVC_E_INVALID_ARG;
    if (n_list < 0 || (n_list > 0 && (!infos || !coef_offsets || !pixel_offsets))) return HVC_E_INVALID_ARG;
    std::vector<const uint16_t *> table_src; // the content behind plan.tables[k]
    unsigned long long units = 0;
    for (int l = 0; l < n_list; l++) {
        const int f = frames ? frames[l] : l;
        if (f < 0) return HVC_E_INVALID_ARG;
        const hvc_jpeg_info &fi = infos[f];
        if (fi.n_comp < 0 || fi.n_comp > 4 || fi.n_qtabs < 0 || fi.n_qtabs > 4) return HVC_E_INVALID_ARG;
        for (int i = 0; i < fi.n_comp; i++) {
            const hvc_component &c = fi.layout[i];
            if (c.blocks_w < 0 || c.blocks_h < 0) return HVC_E_INVALID_ARG;
            if (c.blocks_w == 0 || c.blocks_h == 0) continue; // the model's empty plane: no descriptor, no unit
            if (c.qtab < 0 || c.qtab >= fi.n_qtabs || c.stride < (size_t)c.blocks_w * (size_t)n) return HVC_E_INVALID_ARG;
            const size_t coef_base = coef_offsets[f] + c.coef_offset, pix_base = pixel_offsets[f] + c.plane_offset;
            if ((coef_base & 7) || (n == 8 && ((pix_base & 7) || (c.stride & 7)))) return HVC_E_ALIGNMENT;
            const unsigned long long nblk = (unsigned long long)c.blocks_w * (unsigned long long)c.blocks_h;
            if (nblk * (unsigned long long)c.blocks_w >= (1ull << 32) || nblk >= (1ull << 31)) return HVC_E_TOO_LARGE;
            const unsigned long long nu = (nblk + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT;
            if (units + nu > HVC_MIXED_MAX_UNITS) return HVC_E_TOO_LARGE;
            int t = -1;
            for (size_t k = 0; k < table_src.size() && t < 0; k++)
                if (!std::memcmp(table_src[k], fi.qtabs[c.qtab], 64 * sizeof(uint16_t))) t = (int)k;
            if (t < 0) {
                t = (int)table_src.size();
                table_src.push_back(fi.qtabs[c.qtab]);
                plan.tables.emplace_back();
                table_entry(fi.qtabs[c.qtab], plan.tables.back());
            }
            MixedPlaneK p;
            std::memset(&p, 0, sizeof p);
            p.coef_base = coef_base;
            p.pix_base = pix_base;
            p.stride = c.stride;
            p.bw = c.blocks_w;
            p.nblk = (int)nblk;
            p.magic = c.blocks_w == 1 ? 0u : (unsigned)(((1ull << 32) + (unsigned)c.blocks_w - 1) / (unsigned)c.blocks_w);
            p.table = t;
            p.unit0 = (unsigned)units;
            p.dwords = n != 8 && (((unsigned long long)pix_addr + pix_base) | c.stride) % 4 == 0;
            plan.map.insert(plan.map.end(), (size_t)nu, (unsigned)plan.planes.size());
            plan.planes.push_back(p);
            units += nu;
            plan.blocks += nblk;
        }
    }
    return HVC_OK;
}

// the pair records of the libjpeg-exact block stage, from the entries MixedTableK::qt keeps whole
void mixed_islow_pairs_build(const MixedPlan &plan, std::vector<unsigned> &pairs) {
    pairs.assign(plan.tables.size() * HVC_ISLOW_PAIR_WORDS, 0u);
    for (size_t t = 0; t < plan.tables.size(); t++)
        for (int i = 0; i < HVC_ISLOW_PAIR_WORDS; i++) {
            const int *q = plan.tables[t].qt;
            pairs[t * HVC_ISLOW_PAIR_WORDS + i] = ((unsigned)q[2 * i] & 0xffffu) | ((unsigned)q[2 * i + 1] & 0xffffu) << 16;
        }
}

// hvc_jpeg_mixed_layout (include/hvc_jpeg.h; the entry point itself stands in hvc_capi_jpeg.hip)
int mixed_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, size_t align, hvc_jpeg_info *infos, int *status,
                 size_t *pixel_offsets, size_t *total_bytes) {
    if (!jpegs || !sizes || !infos || !status || !pixel_offsets || !total_bytes || n_files < 0) return HVC_E_INVALID_ARG;
    if (align == 0) align = 256;
    if (align < 8 || (align & (align - 1))) return HVC_E_INVALID_ARG;
    size_t end = 0; // the end of the last record placed
    for (int f = 0; f < n_files; f++) {
        status[f] = jpegs[f] ? hvc_jpeg_read_header(jpegs[f], sizes[f], &infos[f]) : HVC_E_INVALID_ARG;
        const size_t start = (end + align - 1) & ~(align - 1);
        pixel_offsets[f] = start;
        if (status[f] != HVC_OK || infos[f].pixel_bytes == 0) continue; // takes no room
        end = start + infos[f].pixel_bytes;
    }
    *total_bytes = end;
    return HVC_OK;
}

// hvc_jpeg_mixed_scaled_layout (include/hvc_jpeg.h): scale_denom = 1 is mixed_layout itself, with scaled[f] == infos[f]
int mixed_scaled_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int scale_denom, size_t align, hvc_jpeg_info *infos,
                        hvc_jpeg_info *scaled, int *status, size_t *pixel_offsets, size_t *total_bytes) {
    const int n = scaled_side(scale_denom);
    if (!n || !scaled) return HVC_E_INVALID_ARG;
    if (n == 8) {
        const int r = mixed_layout(jpegs, sizes, n_files, align, infos, status, pixel_offsets, total_bytes);
        for (int f = 0; !r && f < n_files; f++)
            if (status[f] == HVC_OK) scaled[f] = infos[f];
        return r;
    }
    if (!jpegs || !sizes || !infos || !status || !pixel_offsets || !total_bytes || n_files < 0) return HVC_E_INVALID_ARG;
    if (align == 0) align = 256;
    if (align < 8 || (align & (align - 1))) return HVC_E_INVALID_ARG;
    size_t end = 0; // the end of the last record placed
    for (int f = 0; f < n_files; f++) {
        status[f] = jpegs[f] ? hvc_jpeg_read_header(jpegs[f], sizes[f], &infos[f]) : HVC_E_INVALID_ARG;
        const size_t start = (end + align - 1) & ~(align - 1);
        pixel_offsets[f] = start;
        if (status[f] != HVC_OK) continue; // takes no room
        scaled_info(infos[f], n, scaled[f]);
        if (scaled[f].pixel_bytes == 0) continue;
        end = start + scaled[f].pixel_bytes;
    }
    *total_bytes = end;
    return HVC_OK;
}

} // namespace hvc
