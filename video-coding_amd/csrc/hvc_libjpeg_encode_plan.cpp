// hvc_libjpeg_encode_plan.cpp -- the division magics and the dummy-block walk of the libjpeg-exact encoder
// (hvc_libjpeg_encode_plan.h).  Plain C++ (no HIP), usable without a GPU.
#include "hvc_libjpeg_encode_plan.h"

#include <algorithm>
#include <cstring>

namespace hvc {

namespace {
// natural position -> zig-zag position (jpeg/model/src/zigzag.ml:71-137)
const unsigned char ZF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                              41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                              46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
} // namespace

uint32_t libjpeg_quant_magic(int q) {
    const uint64_t d = 8u * (uint64_t)q;
    return (uint32_t)((((uint64_t)1 << HVC_LJE_MAGIC_BITS) + d - 1) / d);
}

void libjpeg_encode_tables(const uint16_t *qtabs, int n_qtabs, uint32_t *magic, uint32_t *half) {
    for (int t = 0; t < n_qtabs; t++)
        for (int k = 0; k < 64; k++) {
            const int q = qtabs[t * 64 + ZF[k]];
            magic[t * 64 + k] = libjpeg_quant_magic(q);
            half[t * 64 + k] = 4u * (uint32_t)q;
        }
}

int libjpeg_dummy_source_walk(int bx, int by, int bw, int real_w, int real_h, int h) {
    for (;;) {
        if (by >= real_h) { // the row above, the MCU's last block
            bx = bx / h * h + h - 1;
            by--;
        } else if (bx >= real_w) {
            bx--;
        } else {
            return bx + by * bw;
        }
    }
}

void libjpeg_mixed_tables_build(const std::vector<int> &qt, std::vector<FdctIslowTableK> &tables) {
    tables.assign(qt.size() / 64, FdctIslowTableK());
    for (size_t t = 0; t < tables.size(); t++) {
        uint16_t q[64];
        for (int i = 0; i < 64; i++) q[i] = (uint16_t)qt[t * 64 + (size_t)i];
        libjpeg_encode_tables(q, 1, tables[t].magic, tables[t].half);
    }
}

int libjpeg_mixed_dummies_build(const hvc_jpeg_info *infos, const size_t *coef_offsets, const int *frames, int n_list,
                                std::vector<DummyPairK> &pairs) {
    pairs.clear();
    if (n_list < 0 || (n_list > 0 && (!infos || !coef_offsets))) return HVC_E_INVALID_ARG;
    for (int l = 0; l < n_list; l++) {
        const int f = frames ? frames[l] : l;
        if (f < 0) return HVC_E_INVALID_ARG;
        const hvc_jpeg_info &fi = infos[f];
        if (fi.n_comp < 0 || fi.n_comp > 4) return HVC_E_INVALID_ARG;
        for (int i = 0; i < fi.n_comp; i++) {
            const int bw = fi.layout[i].blocks_w, bh = fi.layout[i].blocks_h, h = fi.comp[i].hscale < 1 ? 1 : fi.comp[i].hscale;
            if (fi.comp[i].actual_width <= 0 || fi.comp[i].actual_height <= 0) continue; // (an info that states no size: every block real)
            const int rw = (fi.comp[i].actual_width + 7) / 8, rh = (fi.comp[i].actual_height + 7) / 8;
            if (rw > bw || rh > bh) return HVC_E_INVALID_ARG;
            const unsigned long long base = (unsigned long long)coef_offsets[f] + fi.layout[i].coef_offset;
            const int n = libjpeg_dummy_count(bw, bh, rw, rh);
            for (int k = 0; k < n; k++) {
                int bx, by;
                libjpeg_dummy_at(k, bw, rw, rh, bx, by);
                pairs.push_back(DummyPairK{base + (unsigned long long)(bx + by * bw) * 64,
                                           base + (unsigned long long)libjpeg_dummy_source(bx, by, bw, rw, rh, h) * 64});
            }
        }
    }
    return HVC_OK;
}

void libjpeg_rgb_lane_grid(int w, int h, int sampling, bool pad, unsigned &lanes_x, unsigned &lanes_y) {
    const bool sub_h = sampling == HVC_YUV_420 || sampling == HVC_YUV_422, sub_v = sampling == HVC_YUV_420;
    const int cw = sub_h ? w / 2 : w, ch = sub_v ? h / 2 : h;
    auto ext = [pad](int x) { return pad ? (x + 7) & ~7 : x; };
    const int full_w = std::max(ext(w), sampling == HVC_YUV_400 ? 0 : (sub_h ? 2 : 1) * ext(cw));
    lanes_x = (unsigned)((full_w + 7) / 8);
    lanes_y = (unsigned)(sub_v ? std::max((ext(h) + 1) / 2, ext(ch)) : ext(h));
}

int libjpeg_rgb_plan_lanes(MixedRgbPlan &plan, bool pad, const hvc_jpeg_info *infos) {
    plan.map.clear();
    plan.lanes = 0;
    unsigned unit = 0;
    for (size_t i = 0; i < plan.images.size(); i++) {
        MixedRgbImageK &k = plan.images[i];
        if (pad) {
            if (!infos || i >= plan.frame.size()) return HVC_E_INVALID_ARG;
            const hvc_jpeg_info &fi = infos[plan.frame[i]];
            const bool sub_h = k.sampling == HVC_YUV_420 || k.sampling == HVC_YUV_422, sub_v = k.sampling == HVC_YUV_420;
            for (int p = 0; p < (k.sampling == HVC_YUV_400 ? 1 : 3); p++) {
                const int aw = p && sub_h ? k.w / 2 : k.w, ah = p && sub_v ? k.h / 2 : k.h;
                const long long ew = (aw + 7) & ~7, eh = (ah + 7) & ~7;
                if (ew > 8LL * fi.layout[p].blocks_w || eh > 8LL * fi.layout[p].blocks_h || (unsigned long long)ew > fi.layout[p].stride)
                    return HVC_E_INVALID_ARG;
            }
        }
        unsigned lx, ly;
        libjpeg_rgb_lane_grid(k.w, k.h, k.sampling, pad, lx, ly);
        const unsigned long long lanes = (unsigned long long)lx * ly;
        if (lanes == 0 || lanes >= (1ull << 31) || (unsigned long long)lx * lanes >= (1ull << 32)) return HVC_E_TOO_LARGE; // (umulhi by magic)
        k.groups = lx;
        k.magic = lx > 1 ? (unsigned)(((1ull << 32) + lx - 1) / lx) : 0u;
        k.lanes = (unsigned)lanes;
        k.unit0 = unit;
        const unsigned units = (unsigned)((lanes + 63) / 64);
        if ((unsigned long long)unit + units > (1u << 26)) return HVC_E_TOO_LARGE;
        plan.map.insert(plan.map.end(), units, (unsigned)i);
        unit += units;
        plan.lanes += lanes;
    }
    return HVC_OK;
}

void pad_plane_replicate(const uint8_t *src, int sw, int sh, uint8_t *dst, int pw, int ph, size_t stride) {
    const int bw = sw < pw ? sw : pw, bh = sh < ph ? sh : ph; // (a plane larger than its padded record is cut, as pad_frame cuts it)
    for (int row = 0; row < ph; row++) {
        uint8_t *d = dst + (size_t)row * stride;
        if (row < bh) {
            std::memcpy(d, src + (size_t)row * sw, (size_t)bw);
            std::memset(d + bw, d[bw - 1], (size_t)(pw - bw));
        } else {
            std::memcpy(d, d - stride, (size_t)pw);
        }
    }
}

void pad_frame_replicate(const hvc_jpeg_info &info, const uint8_t *src, uint8_t *rec) {
    for (int i = 0; i < 3; i++) {
        const hvc_component &L = info.layout[i];
        const int sw = info.comp[i].actual_width, sh = info.comp[i].actual_height;
        const int pw = info.comp[i].decoded_width, ph = info.comp[i].decoded_height;
        if (sw > 0 && sh > 0) pad_plane_replicate(src, sw, sh, rec + L.plane_offset, pw, ph, L.stride);
        else // (nothing to repeat: zeros, as pad_frame)
            for (int row = 0; row < ph; row++) std::memset(rec + L.plane_offset + (size_t)row * L.stride, 0, (size_t)pw);
        src += (size_t)sw * sh;
    }
}

} // namespace hvc
