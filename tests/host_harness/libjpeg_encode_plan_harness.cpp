// libjpeg_encode_plan_harness.cpp -- the host arithmetic of the libjpeg-exact encoder (csrc/hvc_libjpeg_encode_plan.cpp)
// without a GPU, under AddressSanitizer and UndefinedBehaviorSanitizer (Makefile.libjpeg_encode; driven by
// tests/test_libjpeg_encode_plan.py).
//   magics            every q in 1 .. HVC_FI_Q_MAX against every |t| in 0 .. HVC_FI_T_MAX, both signs: the multiplier's quotient
//                     and libjpeg_quantise against C's / on the definition sign(t) * ((|t| + 4 q) / (8 q))
//   tables            libjpeg_encode_tables of a ramp table: natural-order words of zig-zag entries (printed)
//   dummies BW BH     every plane up to BW x BH blocks, every sampling factor 1 .. 4, every real size the factors allow: the
//                     closed form against the walk for every block, the enumeration of the dummies against a scan
//   rgb               the lane grid of the colour pass (libjpeg_rgb_lane_grid, libjpeg_rgb_plan_lanes): every size up to 70 x 40, every
//                     sampling, padded or not -- the grid covers every component's extent and no more than 7 columns / a row pair
//                     beyond it, units and map are consistent, the reciprocal finds every lane's row, a padded component that does
//                     not fit its plane is refused
//   pad               pad_frame_replicate into records of exactly the layout's size (the sanitizer sees one byte too many)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hvc_libjpeg_encode_plan.h"

static int fail(const char *what, long a, long b, long c) {
    std::printf("FAIL %s %ld %ld %ld\n", what, a, b, c);
    return 1;
}

static int magics() {
    unsigned long long checked = 0;
    for (int q = 1; q <= HVC_FI_Q_MAX; q++) {
        const uint32_t m = hvc::libjpeg_quant_magic(q), half = 4u * (uint32_t)q, d = 8u * (uint32_t)q;
        if ((unsigned long long)m * d < (1ull << HVC_LJE_MAGIC_BITS) || (unsigned long long)m * d >= (1ull << HVC_LJE_MAGIC_BITS) + d ||
            m >= (1u << 24) || ((HVC_FI_T_MAX + half) << HVC_LJE_NUMERATOR_SHIFT) >= (1u << 24))
            return fail("magic", q, m, 0); // (both factors of the kernel's product in 24 bits)
        for (int t = 0; t <= HVC_FI_T_MAX; t++) {
            const uint32_t want = ((uint32_t)t + half) / d;
            if (hvc::libjpeg_quant_divide((uint32_t)t + half, m) != want) return fail("divide", q, t, want);
            // the kernel's form of it: the high dword of ((n << shift) & 0xffffff) * (m & 0xffffff)
            const unsigned long long n24 = (((uint32_t)t + half) << HVC_LJE_NUMERATOR_SHIFT) & 0xffffffu;
            if ((uint32_t)((n24 * (m & 0xffffffu)) >> 32) != want) return fail("mul_hi_u24", q, t, want);
            if (hvc::libjpeg_quantise(t, m, half) != (int)want || hvc::libjpeg_quantise(-t, m, half) != -(int)want)
                return fail("quantise", q, t, want);
            checked += 2;
        }
    }
    std::printf("ok magics %llu\n", checked);
    return 0;
}

static int tables() {
    uint16_t q[2 * 64];
    for (int i = 0; i < 64; i++) {
        q[i] = (uint16_t)(i + 1);       // zig-zag position i holds i + 1
        q[64 + i] = (uint16_t)(255 - i);
    }
    uint32_t magic[2 * 64], half[2 * 64];
    hvc::libjpeg_encode_tables(q, 2, magic, half);
    std::printf("tables");
    for (int i = 0; i < 2 * 64; i++) std::printf(" %u %u", magic[i], half[i]);
    std::printf("\n");
    return 0;
}

static int dummies(int max_bw, int max_bh) {
    unsigned long long planes = 0, blocks = 0;
    for (int h = 1; h <= 4; h++)
        for (int v = 1; v <= 4; v++)
            for (int bw = h; bw <= max_bw; bw += h)
                for (int bh = v; bh <= max_bh; bh += v)
                    for (int rw = bw - h + 1; rw <= bw; rw++)
                        for (int rh = bh - v + 1; rh <= bh; rh++) {
                            planes++;
                            std::vector<int> seen((size_t)bw * bh, 0);
                            const int n = hvc::libjpeg_dummy_count(bw, bh, rw, rh);
                            for (int i = 0; i < n; i++) {
                                int bx = -1, by = -1;
                                hvc::libjpeg_dummy_at(i, bw, rw, rh, bx, by);
                                if (bx < 0 || bx >= bw || by < 0 || by >= bh || (bx < rw && by < rh)) return fail("dummy_at", i, bx, by);
                                if (seen[(size_t)by * bw + bx]++) return fail("dummy twice", i, bx, by);
                            }
                            for (int by = 0; by < bh; by++)
                                for (int bx = 0; bx < bw; bx++) {
                                    blocks++;
                                    const bool real = bx < rw && by < rh;
                                    if (!real && !seen[(size_t)by * bw + bx]) return fail("dummy missed", bx, by, bw);
                                    const int want = hvc::libjpeg_dummy_source_walk(bx, by, bw, rw, rh, h);
                                    const int got = hvc::libjpeg_dummy_source(bx, by, bw, rw, rh, h);
                                    if (got != want) return fail("source", bx + 1000 * by, got, want);
                                    if (real && got != bx + by * bw) return fail("real", bx, by, got);
                                    if (want % bw >= rw || want / bw >= rh) return fail("source is a dummy", bx, by, want);
                                }
                        }
    std::printf("ok dummies %llu %llu\n", planes, blocks);
    return 0;
}

static int pad() {
    unsigned long long frames = 0;
    static const int S[3][6] = {{2, 2, 1, 1, 1, 1}, {2, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1}};
    for (int s = 0; s < 3; s++)
        for (int w = 2; w <= 40; w++)
            for (int hgt = 2; hgt <= 35; hgt += (hgt < 18 ? 1 : 7)) {
                hvc_jpeg_info info;
                std::memset(&info, 0, sizeof info);
                size_t off = 0, in = 0;
                for (int i = 0; i < 3; i++) {
                    hvc_jpeg_component &c = info.comp[i];
                    c.hscale = S[s][2 * i];
                    c.vscale = S[s][2 * i + 1];
                    c.actual_width = w * c.hscale / S[s][0];
                    c.actual_height = hgt * c.vscale / S[s][1];
                    c.decoded_width = (c.actual_width + 8 * c.hscale - 1) / (8 * c.hscale) * (8 * c.hscale);
                    c.decoded_height = (c.actual_height + 8 * c.vscale - 1) / (8 * c.vscale) * (8 * c.vscale);
                    info.layout[i].plane_offset = off;
                    info.layout[i].stride = (size_t)c.decoded_width;
                    off += (size_t)c.decoded_width * c.decoded_height;
                    in += (size_t)c.actual_width * c.actual_height;
                }
                std::vector<uint8_t> src(in), rec(off, 0xA5);
                for (size_t i = 0; i < in; i++) src[i] = (uint8_t)(i * 37 + w + 3 * hgt);
                hvc::pad_frame_replicate(info, src.data(), rec.data());
                const uint8_t *p = src.data();
                for (int i = 0; i < 3; i++) {
                    const hvc_jpeg_component &c = info.comp[i];
                    for (int y = 0; y < c.decoded_height; y++)
                        for (int x = 0; x < c.decoded_width; x++) {
                            const int sx = x < c.actual_width ? x : c.actual_width - 1, sy = y < c.actual_height ? y : c.actual_height - 1;
                            if (rec[info.layout[i].plane_offset + (size_t)y * info.layout[i].stride + x] != p[(size_t)sy * c.actual_width + sx])
                                return fail("pad", i, x, y);
                        }
                    p += (size_t)c.actual_width * c.actual_height;
                }
                frames++;
            }
    std::printf("ok pad %llu\n", frames);
    return 0;
}

static int rgb() {
    unsigned long long images = 0;
    static const int S[4] = {HVC_YUV_420, HVC_YUV_422, HVC_YUV_444, HVC_YUV_400};
    for (int pad = 0; pad < 2; pad++) {
        hvc::MixedRgbPlan plan;
        std::vector<hvc_jpeg_info> infos;
        for (int s = 0; s < 4; s++)
            for (int w = 1; w <= 70; w++)
                for (int h = 1; h <= 40; h++) {
                    const bool sub_h = S[s] == HVC_YUV_420 || S[s] == HVC_YUV_422, sub_v = S[s] == HVC_YUV_420;
                    if ((sub_h && (w & 1)) || (sub_v && (h & 1))) continue;
                    hvc::MixedRgbImageK k;
                    std::memset(&k, 0, sizeof k);
                    k.w = w, k.h = h, k.sampling = S[s];
                    plan.images.push_back(k);
                    plan.frame.push_back((int)infos.size());
                    hvc_jpeg_info fi;
                    std::memset(&fi, 0, sizeof fi);
                    for (int p = 0; p < 3; p++) {
                        const int aw = p && sub_h ? w / 2 : w, ah = p && sub_v ? h / 2 : h;
                        fi.layout[p].blocks_w = (aw + 7) / 8, fi.layout[p].blocks_h = (ah + 7) / 8;
                        fi.layout[p].stride = (size_t)fi.layout[p].blocks_w * 8;
                    }
                    infos.push_back(fi);
                }
        if (hvc::libjpeg_rgb_plan_lanes(plan, pad != 0, infos.data()) != HVC_OK) return fail("plan", pad, 0, 0);
        unsigned unit = 0;
        for (size_t i = 0; i < plan.images.size(); i++) {
            const hvc::MixedRgbImageK &k = plan.images[i];
            const bool sub_h = k.sampling == HVC_YUV_420 || k.sampling == HVC_YUV_422, sub_v = k.sampling == HVC_YUV_420;
            const int cw = sub_h ? k.w / 2 : k.w, ch = sub_v ? k.h / 2 : k.h;
            const int ewy = pad ? (k.w + 7) & ~7 : k.w, ehy = pad ? (k.h + 7) & ~7 : k.h, ewc = pad ? (cw + 7) & ~7 : cw, ehc = pad ? (ch + 7) & ~7 : ch;
            const int lx = (int)k.groups, ly = (int)(k.lanes / k.groups);
            const bool grey = k.sampling == HVC_YUV_400;
            const int need_x = std::max(ewy, grey ? 0 : (sub_h ? 2 : 1) * ewc), need_y = sub_v ? std::max((ehy + 1) / 2, ehc) : ehy;
            if (k.lanes != k.groups * (unsigned)ly || lx * 8 < need_x || lx * 8 >= need_x + 8 || ly != need_y) return fail("grid", k.w, k.h, k.sampling);
            if (k.unit0 != unit) return fail("unit0", (long)i, k.unit0, unit);
            for (unsigned u = 0; u < (k.lanes + 63) / 64; u++)
                if (plan.map[unit + u] != i) return fail("map", (long)i, u, 0);
            unit += (k.lanes + 63) / 64;
            for (unsigned lane = 0; lane < k.lanes; lane++) {
                const unsigned row = k.groups == 1 ? lane : (unsigned)(((unsigned long long)lane * k.magic) >> 32);
                if (row != lane / k.groups) return fail("magic", k.groups, lane, row);
            }
            images++;
        }
        if (unit != plan.map.size()) return fail("units", unit, (long)plan.map.size(), 0);
        if (pad) { // a plane one block too narrow, then one too low
            hvc::MixedRgbPlan one;
            one.images.push_back(plan.images[0]);
            one.images[0].w = 18, one.images[0].h = 10, one.images[0].sampling = HVC_YUV_420;
            one.frame.push_back(0);
            hvc_jpeg_info fi = infos[0];
            fi.layout[0].blocks_w = 3, fi.layout[0].blocks_h = 2, fi.layout[0].stride = 24;
            fi.layout[1] = fi.layout[2] = fi.layout[0];
            fi.layout[1].blocks_w = fi.layout[2].blocks_w = 2, fi.layout[1].blocks_h = fi.layout[2].blocks_h = 1;
            if (hvc::libjpeg_rgb_plan_lanes(one, true, &fi) != HVC_OK) return fail("fits", 0, 0, 0);
            fi.layout[1].blocks_w = 1;
            if (hvc::libjpeg_rgb_plan_lanes(one, true, &fi) != HVC_E_INVALID_ARG) return fail("narrow", 0, 0, 0);
            fi.layout[1].blocks_w = 2, fi.layout[0].blocks_h = 1;
            if (hvc::libjpeg_rgb_plan_lanes(one, true, &fi) != HVC_E_INVALID_ARG) return fail("low", 0, 0, 0);
        }
    }
    std::printf("ok rgb %llu\n", images);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "magics")) return magics();
    if (argc >= 2 && !std::strcmp(argv[1], "tables")) return tables();
    if (argc >= 4 && !std::strcmp(argv[1], "dummies")) return dummies(std::atoi(argv[2]), std::atoi(argv[3]));
    if (argc >= 2 && !std::strcmp(argv[1], "pad")) return pad();
    if (argc >= 2 && !std::strcmp(argv[1], "rgb")) return rgb();
    std::printf("usage: magics | tables | dummies BW BH | pad | rgb\n");
    return 2;
}
