// Stand-alone driver of hvc::mixed_rgb_encode_plan_build (csrc/hvc_mixed_rgb_plan.cpp) for tests/test_mixed_rgb_encode_plan.py,
// built by Makefile.mixed_rgb_encode with -fsanitize=address,undefined (CPU only, no device code):
//   mixed_rgb_encode_plan_harness dump FILE          FILE = int64 n_frames, n_list (-1: no list), layout, yuv_addr, rgb_addr,
//                                                    has_strides; hvc_jpeg_info[n_frames]; uint64 yuv_offsets[n_frames],
//                                                    rgb_offsets[n_frames], rgb_row_strides[n_frames]; int32 list[n_list];
//                                                    prints the plan, and what check_plan here says of it
//   mixed_rgb_encode_plan_harness random SEED COUNT  COUNT seeded random sets of even-sized frames, each checked here: every
//                                                    lane of every listed image lies in exactly one (unit, lane), the flags
//                                                    follow the addresses; one set in ten is spoilt by an odd size
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hvc_mixed_rgb_plan.h"

namespace {

struct Set {
    std::vector<hvc_jpeg_info> infos;
    std::vector<size_t> yuv, rgb, strides;
    std::vector<int> list;
    bool has_list = false, has_strides = true;
    int layout = 0;
    uintptr_t yuv_addr = 0, rgb_addr = 0;
};

bool read_all(const char *path, std::vector<unsigned char> &out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

int sampling_by_factors(const hvc_jpeg_info &fi) { // the rule, written again
    if (fi.n_comp != 3) return 0;
    const int h0 = fi.comp[0].hscale, v0 = fi.comp[0].vscale, h1 = fi.comp[1].hscale, v1 = fi.comp[1].vscale;
    if (fi.comp[2].hscale != h1 || fi.comp[2].vscale != v1 || h1 < 1 || v1 < 1) return 0;
    if (h0 == h1 && v0 == v1) return 444;
    if (h0 == 2 * h1 && v0 == 2 * v1) return 420;
    if (h0 == 2 * h1 && v0 == v1) return 422;
    return 0;
}

// the properties every plan of the encode direction must have; returns an empty string or what is wrong
std::string check_plan(const Set &s, const hvc::MixedRgbPlan &plan) {
    const int n_list = s.has_list ? (int)s.list.size() : (int)s.infos.size();
    size_t pi = 0;
    unsigned long long units = 0, lanes_total = 0;
    for (int l = 0; l < n_list; l++) {
        const int f = s.has_list ? s.list[(size_t)l] : l;
        const hvc_jpeg_info &fi = s.infos[(size_t)f];
        if (fi.width == 0 || fi.height == 0) continue;
        if (pi >= plan.images.size()) return "an image without a descriptor";
        const hvc::MixedRgbImageK &k = plan.images[pi];
        if (plan.frame[pi] != f) return "frame index";
        const int sampling = sampling_by_factors(fi);
        if (k.w != fi.width || k.h != fi.height || k.sampling != sampling) return "geometry";
        if (k.cw != (sampling == 444 ? k.w : k.w / 2) || k.ch != (sampling == 420 ? k.h / 2 : k.h)) return "chroma size";
        const unsigned groups = ((unsigned)k.w + 7) / 8, lrows = sampling == 420 ? (unsigned)k.h / 2 : (unsigned)k.h;
        if (k.groups != groups || k.lanes != groups * lrows) return "lanes";
        if (k.y_base != s.yuv[(size_t)f] + fi.layout[0].plane_offset || k.y_stride != fi.layout[0].stride) return "luma base";
        if (k.cb_base != s.yuv[(size_t)f] + fi.layout[1].plane_offset || k.cr_base != s.yuv[(size_t)f] + fi.layout[2].plane_offset ||
            k.cb_stride != fi.layout[1].stride || k.cr_stride != fi.layout[2].stride)
            return "chroma bases";
        const size_t tight = s.layout == HVC_RGB_PLANAR ? (size_t)k.w : (size_t)3 * k.w;
        const size_t rs = s.has_strides && s.strides[(size_t)f] ? s.strides[(size_t)f] : tight;
        if (k.rgb_base != s.rgb[(size_t)f] || k.row_stride != rs || k.plane_stride != rs * (size_t)k.h) return "rgb base";
        // the flags by the actual addresses: every row of every plane / of the image starts on the boundary
        bool vy = true, vc = true, vr = true;
        for (int row = 0; row < k.h && row < 4; row++) vy &= (s.yuv_addr + k.y_base + (size_t)row * k.y_stride) % 8 == 0;
        for (int row = 0; row < k.ch && row < 4; row++) {
            const size_t a = sampling == 444 ? 8 : 4;
            vc &= (s.yuv_addr + k.cb_base + (size_t)row * k.cb_stride) % a == 0 && (s.yuv_addr + k.cr_base + (size_t)row * k.cr_stride) % a == 0;
        }
        for (int p = 0; p < (s.layout == HVC_RGB_PLANAR ? 3 : 1); p++)
            for (int row = 0; row < k.h && row < 4; row++) vr &= (s.rgb_addr + k.rgb_base + (size_t)p * k.plane_stride + (size_t)row * k.row_stride) % 8 == 0;
        // (a one-row plane whose stride is off the boundary has every row aligned: the flag may still be 0, never wrongly 1)
        if ((k.vec_y && !vy) || (k.vec_c && !vc) || (k.vec_rgb && !vr)) return "a flag set for rows off their boundary";
        if (k.h >= 2 && ((k.vec_y != 0) != vy || (k.ch >= 2 && (k.vec_c != 0) != vc) || (k.vec_rgb != 0) != vr)) return "a flag not set";
        if (k.unit0 != units) return "unit0";
        // every lane in exactly one (unit, lane): the kernel's t = (unit - unit0) * 64 + lane, lr = umulhi(t, magic); and the
        // samples the lane touches lie inside the image: rows ROWS * lr .. < h, chroma row lr < ch
        std::vector<unsigned char> seen((size_t)k.lanes, 0);
        const unsigned long long nu = ((unsigned long long)k.lanes + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT;
        for (unsigned long long u = units; u < units + nu; u++) {
            if (u >= plan.map.size() || plan.map[(size_t)u] != pi) return "map entry";
            for (int lane = 0; lane < HVC_MIXED_UNIT; lane++) {
                const unsigned long long t = (u - k.unit0) * HVC_MIXED_UNIT + (unsigned)lane;
                if (t >= k.lanes) continue;
                const unsigned lr = k.groups == 1 ? (unsigned)t : (unsigned)(((unsigned long long)(unsigned)t * k.magic) >> 32);
                const unsigned g = (unsigned)t - lr * k.groups;
                if (g >= groups || lr >= lrows) return "lane position";
                const unsigned rows = sampling == 420 ? 2 : 1;
                if (lr * rows + rows > (unsigned)k.h || lr >= (unsigned)k.ch || 8 * g >= (unsigned)k.w) return "a lane outside its image";
                if (seen[(size_t)lr * groups + g]++) return "a lane twice";
            }
        }
        for (unsigned char v : seen)
            if (v != 1) return "a lane without a unit";
        units += nu;
        lanes_total += k.lanes;
        pi++;
    }
    if (pi != plan.images.size() || units != plan.map.size() || lanes_total != plan.lanes) return "totals";
    return "";
}

int build(const Set &s, hvc::MixedRgbPlan &plan) {
    return hvc::mixed_rgb_encode_plan_build(s.infos.data(), s.yuv.data(), s.rgb.data(), s.has_strides ? s.strides.data() : nullptr, s.layout,
                                            s.has_list ? s.list.data() : nullptr, s.has_list ? (int)s.list.size() : (int)s.infos.size(),
                                            s.yuv_addr, s.rgb_addr, plan);
}

int cmd_dump(const char *path) {
    std::vector<unsigned char> raw;
    if (!read_all(path, raw) || raw.size() < 48) return 2;
    long long h[6];
    std::memcpy(h, raw.data(), sizeof h);
    const long long n = h[0], nl = h[1];
    Set s;
    s.layout = (int)h[2], s.yuv_addr = (uintptr_t)h[3], s.rgb_addr = (uintptr_t)h[4], s.has_strides = h[5] != 0;
    size_t at = sizeof h;
    if (n < 0 || raw.size() != at + (size_t)n * (sizeof(hvc_jpeg_info) + 24) + (nl > 0 ? (size_t)nl * 4 : 0)) return 2;
    s.infos.resize((size_t)n);
    s.yuv.resize((size_t)n);
    s.rgb.resize((size_t)n);
    s.strides.resize((size_t)n);
    if (n) std::memcpy(s.infos.data(), raw.data() + at, (size_t)n * sizeof(hvc_jpeg_info));
    at += (size_t)n * sizeof(hvc_jpeg_info);
    for (long long i = 0; i < n; i++) {
        unsigned long long v;
        std::memcpy(&v, raw.data() + at + 8 * (size_t)i, 8);
        s.yuv[(size_t)i] = (size_t)v;
        std::memcpy(&v, raw.data() + at + 8 * (size_t)(n + i), 8);
        s.rgb[(size_t)i] = (size_t)v;
        std::memcpy(&v, raw.data() + at + 8 * (size_t)(2 * n + i), 8);
        s.strides[(size_t)i] = (size_t)v;
    }
    at += 24 * (size_t)n;
    if (nl >= 0) {
        s.has_list = true;
        s.list.resize((size_t)nl);
        if (nl) std::memcpy(s.list.data(), raw.data() + at, (size_t)nl * 4);
        for (int f : s.list)
            if (f < 0 || f >= n) return 2;
    }
    hvc::MixedRgbPlan plan;
    const int r = build(s, plan);
    std::printf("status %d\n", r);
    if (r) {
        if (!plan.images.empty() || !plan.map.empty()) std::printf("check a refused plan holds tables\n");
        return 0;
    }
    const std::string bad = check_plan(s, plan);
    std::printf("check %s\n", bad.empty() ? "ok" : bad.c_str());
    std::printf("lanes %llu\n", plan.lanes);
    for (size_t i = 0; i < plan.images.size(); i++) {
        const hvc::MixedRgbImageK &k = plan.images[i];
        std::printf("image %zu %d %llu %llu %llu %llu %llu %llu %llu %llu %llu %d %d %d %d %d %d %d %d %u %u %u %u\n", i, plan.frame[i], k.y_base,
                    k.cb_base, k.cr_base, k.rgb_base, k.y_stride, k.cb_stride, k.cr_stride, k.row_stride, k.plane_stride, k.w, k.h, k.cw, k.ch,
                    k.sampling, k.vec_y, k.vec_c, k.vec_rgb, k.groups, k.magic, k.lanes, k.unit0);
    }
    std::printf("map");
    for (unsigned u : plan.map) std::printf(" %u", u);
    std::printf("\n");
    return 0;
}

unsigned long long rng_state;
unsigned rnd(unsigned n) { // splitmix64
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) % n);
}

int cmd_random(unsigned long long seed, int count) {
    rng_state = seed;
    static const int SIDES[] = {0, 2, 4, 6, 8, 10, 14, 16, 18, 62, 64, 66, 72, 254, 256, 258, 520, 2050};
    static const int SAMPLINGS[] = {420, 422, 444};
    const unsigned NS = sizeof SIDES / sizeof SIDES[0];
    int refused = 0;
    for (int it = 0; it < count; it++) {
        Set s;
        s.layout = (int)rnd(2);
        s.yuv_addr = (uintptr_t)0x7f0000000000ull + (rnd(4) ? 0 : rnd(8));
        s.rgb_addr = (uintptr_t)0x7e0000000000ull + (rnd(4) ? 0 : rnd(8));
        s.has_strides = rnd(3) != 0;
        const int n = 1 + (int)rnd(12);
        size_t yuv = 0, rgb = 0;
        for (int f = 0; f < n; f++) {
            hvc_jpeg_info fi;
            std::memset(&fi, 0, sizeof fi);
            const int sampling = SAMPLINGS[rnd(3)];
            fi.width = SIDES[rnd(NS)] + (sampling == 444 ? (int)rnd(2) : 0); // (4:4:4 takes odd sizes)
            fi.height = (rnd(3) ? SIDES[rnd(NS)] : 2 * (1 + (int)rnd(3))) + (sampling != 420 ? (int)rnd(2) : 0);
            fi.n_comp = 3;
            const int hs = sampling == 444 ? 1 : 2, vs = sampling == 420 ? 2 : 1;
            size_t po = 0;
            for (int i = 0; i < 3; i++) {
                fi.comp[i].hscale = i ? 1 : hs, fi.comp[i].vscale = i ? 1 : vs;
                hvc_component &c = fi.layout[i];
                const int pw = i && hs == 2 ? fi.width / 2 : fi.width, ph = i && vs == 2 ? fi.height / 2 : fi.height;
                c.blocks_w = (pw + 7) / 8 + (int)rnd(2), c.blocks_h = (ph + 7) / 8 + (int)rnd(2);
                c.stride = rnd(4) ? (size_t)c.blocks_w * 8 : (size_t)pw + rnd(7); // (padded planes, or raw ones at any stride)
                c.plane_offset = po + (rnd(6) ? 0 : rnd(8));
                po = c.plane_offset + c.stride * (size_t)(c.blocks_h * 8);
            }
            fi.pixel_bytes = po;
            const size_t tight = s.layout == HVC_RGB_PLANAR ? (size_t)fi.width : (size_t)3 * fi.width;
            const size_t rs = rnd(2) ? 0 : (tight + 7 + rnd(9)) & ~(size_t)(rnd(2) ? 7 : 0);
            s.infos.push_back(fi);
            s.yuv.push_back(yuv);
            s.rgb.push_back(rgb);
            s.strides.push_back(rs);
            yuv += (po + (rnd(2) ? 255 : 0)) & ~(size_t)(rnd(2) ? 255 : 0);
            rgb += (rs ? rs : tight) * (size_t)fi.height * (s.layout == HVC_RGB_PLANAR ? 3 : 1) + rnd(3);
        }
        if (rnd(2)) { // a list with holes
            s.has_list = true;
            for (int f = 0; f < n; f++)
                if (rnd(4)) s.list.push_back(f);
        }
        bool spoil = rnd(10) == 0;
        if (spoil) { // an odd width under 4:2:0 / 4:2:2 in a listed frame
            const int f = s.has_list ? (s.list.empty() ? -1 : s.list[rnd((unsigned)s.list.size())]) : (int)rnd((unsigned)n);
            if (f < 0 || sampling_by_factors(s.infos[(size_t)f]) == 444)
                spoil = false;
            else
                s.infos[(size_t)f].width += 1;
        }
        hvc::MixedRgbPlan plan;
        const int r = build(s, plan);
        if (r) {
            if (!(spoil && r == HVC_E_INVALID_ARG)) {
                std::printf("set %d: status %d\n", it, r);
                return 1;
            }
            refused++;
            continue;
        }
        if (spoil) {
            std::printf("set %d: an odd width accepted\n", it);
            return 1;
        }
        const std::string bad = check_plan(s, plan);
        if (!bad.empty()) {
            std::printf("set %d: %s\n", it, bad.c_str());
            return 1;
        }
    }
    std::printf("ok %d refused %d\n", count, refused);
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "dump")) return cmd_dump(argv[2]);
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return cmd_random(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    std::fprintf(stderr, "usage: mixed_rgb_encode_plan_harness dump FILE | random SEED COUNT\n");
    return 2;
}
