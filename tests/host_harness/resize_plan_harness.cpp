// Stand-alone driver of csrc/hvc_resize_plan.cpp for tests/test_resize_plan.py, built by Makefile.resize with
// -fsanitize=address,undefined and -ffp-contract=off (CPU only, no device code):
//   resize_plan_harness sweep OUT N_IN... -- N_OUT...   every (n_in, n_out, filter) of the two lists under the three filters:
//                                             OUT receives, per table, int32 n_in, n_out, filter, status, kmax, then (status 0)
//                                             xmin[n_out], count[n_out], first[n_out], taps[kmax * n_out] as the plan stores them
//   resize_plan_harness plan FILE             FILE = int64 n_images, n_list (-1: no list), layout, filter, src_addr, dst_addr;
//                                             per image int64 w, h, out_w, out_h, src_offset, src_row_stride, dst_offset,
//                                             dst_row_stride; int32 list[n_list]; prints the plan hvc::resize_plan_build makes
//   resize_plan_harness random SEED COUNT     COUNT seeded random sets, each checked here: every lane of every pass lies in
//                                             exactly one (unit, lane), every access stays inside its image or intermediate
//   resize_plan_harness status W H OUT_W OUT_H FILTER   hvc::resize_image_status
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hvc_resize_plan.h"

namespace {

bool read_all(const char *path, std::vector<unsigned char> &out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

int cmd_sweep(const char *out_path, int argc, char **argv) {
    std::vector<int> ins, outs;
    bool second = false;
    for (int i = 0; i < argc; i++) {
        if (!std::strcmp(argv[i], "--")) {
            second = true;
            continue;
        }
        (second ? outs : ins).push_back(std::atoi(argv[i]));
    }
    FILE *f = std::fopen(out_path, "wb");
    if (!f) return 2;
    long long tables = 0, worst = 0;
    for (int n_in : ins)
        for (int n_out : outs)
            for (int filter = 0; filter < 3; filter++) {
                std::vector<hvc::ResizeRecK> recs;
                std::vector<int> taps;
                const int r = hvc::resize_axis_build(n_in, n_out, filter, recs, taps);
                const int kmax = r || n_out < 1 ? 0 : (int)(taps.size() / (size_t)n_out);
                const int head[5] = {n_in, n_out, filter, r, kmax};
                std::fwrite(head, sizeof head, 1, f);
                tables++;
                if (r) continue;
                std::vector<int> col((size_t)n_out);
                for (int p = 0; p < n_out; p++) col[(size_t)p] = (int)recs[(size_t)p].xmin;
                std::fwrite(col.data(), 4, col.size(), f);
                for (int p = 0; p < n_out; p++) col[(size_t)p] = (int)recs[(size_t)p].count;
                std::fwrite(col.data(), 4, col.size(), f);
                for (int p = 0; p < n_out; p++) col[(size_t)p] = (int)recs[(size_t)p].first;
                std::fwrite(col.data(), 4, col.size(), f);
                if (!taps.empty()) std::fwrite(taps.data(), 4, taps.size(), f);
                // the overflow check, again: 255 * SUM |k| + 2^21 < 2^31 at every position
                for (int p = 0; p < n_out; p++) {
                    long long s = 0;
                    for (unsigned i = 0; i < recs[(size_t)p].count; i++) {
                        const long long k = taps[(size_t)i * (size_t)n_out + (size_t)p];
                        s += k < 0 ? -k : k;
                    }
                    if (s > worst) worst = s;
                    if (255 * s + (1ll << 21) >= (1ll << 31)) {
                        std::printf("overflow %d %d %d %d\n", n_in, n_out, filter, p);
                        std::fclose(f);
                        return 1;
                    }
                }
            }
    std::fclose(f);
    std::printf("ok %lld worst %lld\n", tables, worst);
    return 0;
}

struct Set {
    std::vector<hvc::ResizeImage> images;
    std::vector<int> list;
    bool has_list = false;
    int layout = 0, filter = 0;
    uintptr_t src_addr = 0, dst_addr = 0;
};

int build(const Set &s, hvc::ResizePlan &plan) {
    return hvc::resize_plan_build(s.images.data(), s.has_list ? s.list.data() : nullptr, s.has_list ? (int)s.list.size() : (int)s.images.size(),
                                  s.layout, s.filter, s.src_addr, s.dst_addr, plan);
}

// the properties every plan must have; returns an empty string or what is wrong
std::string check_plan(const Set &s, const hvc::ResizePlan &plan) {
    const int n_list = s.has_list ? (int)s.list.size() : (int)s.images.size();
    const unsigned planes = s.layout == HVC_RGB_PLANAR ? 3 : 1, ch = s.layout == HVC_RGB_PLANAR ? 1 : 3;
    size_t hi = 0, vi = 0;
    unsigned long long hu = 0, vu = 0;
    for (int l = 0; l < n_list; l++) {
        const int f = s.has_list ? s.list[(size_t)l] : l;
        const hvc::ResizeImage &im = s.images[(size_t)f];
        const bool need_h = im.out_w != im.w, need_v = im.out_h != im.h || !need_h, both = need_h && need_v;
        const unsigned long long st = hvc::resize_row_bytes(s.layout, im.w), dt = hvc::resize_row_bytes(s.layout, im.out_w);
        const unsigned long long ss = im.src_row_stride ? im.src_row_stride : st, ds = im.dst_row_stride ? im.dst_row_stride : dt;
        for (unsigned p = 0; p < planes; p++) {
            if (need_h) {
                if (hi >= plan.h.images.size()) return "an image without a horizontal descriptor";
                const hvc::ResizeImageK &k = plan.h.images[hi];
                if (plan.h.image[hi] != f) return "h: image index";
                if (k.ch != ch || k.n_out != (unsigned)im.out_w || k.rows != (unsigned)im.h || k.groups != (unsigned)im.out_w) return "h: geometry";
                if (k.lanes != (unsigned)im.out_w * (unsigned)im.h || k.tap_stride != (unsigned)im.out_w) return "h: lanes";
                if (k.src_sel != 0 || k.dst_sel != (both ? 1u : 0u)) return "h: selectors";
                if (k.src_base != im.src_offset + p * ss * (unsigned long long)im.h || k.src_stride != ss) return "h: source";
                if (!both && (k.dst_base != im.dst_offset + p * ds * (unsigned long long)im.out_h || k.dst_stride != ds)) return "h: destination";
                if (both && (k.dst_base % 64 != 0 && p == 0)) return "h: intermediate off 64 bytes";
                if (both && (k.dst_stride % 4 != 0 || k.dst_stride < dt || k.dst_base + k.dst_stride * (unsigned long long)im.h > plan.mid_bytes)) return "h: intermediate";
                if (k.unit0 != hu || k.units != (k.lanes + 63) / 64) return "h: units";
                std::vector<unsigned char> seen((size_t)k.lanes, 0);
                for (unsigned long long u = hu; u < hu + k.units; u++) {
                    if (u >= plan.h.map.size() || plan.h.map[(size_t)u] != hi) return "h: map entry";
                    for (unsigned lane = 0; lane < 64; lane++) {
                        const unsigned long long t = (u - k.unit0) * 64 + lane;
                        if (t >= k.lanes) continue;
                        const unsigned row = k.groups == 1 ? (unsigned)t : (unsigned)(((unsigned long long)(unsigned)t * k.magic) >> 32);
                        const unsigned xx = (unsigned)t - row * k.groups;
                        if (xx >= k.n_out || row >= k.rows) return "h: lane position";
                        if (seen[(size_t)row * k.n_out + xx]++) return "h: a lane twice";
                        const hvc::ResizeRecK &rec = plan.recs[k.rec0 + xx];
                        if (rec.xmin + rec.count > (unsigned)im.w) return "h: a window beyond the row";
                        if (rec.count && (size_t)rec.first + (size_t)(rec.count - 1) * k.tap_stride >= plan.taps.size()) return "h: a tap beyond the table";
                    }
                }
                for (unsigned char v : seen)
                    if (v != 1) return "h: a lane without a unit";
                hu += k.units;
                hi++;
            }
            if (need_v) {
                if (vi >= plan.v.images.size()) return "an image without a vertical descriptor";
                const hvc::ResizeImageK &k = plan.v.images[vi];
                if (plan.v.image[vi] != f) return "v: image index";
                if (k.n_out != (unsigned)im.out_h || k.rows != (unsigned)im.h || k.row_bytes != dt || k.tap_stride != (unsigned)im.out_h) return "v: geometry";
                if (k.lanes != (k.row_bytes + 3) / 4 || k.groups != (k.lanes + 63) / 64 || k.units != k.groups * k.n_out) return "v: lanes";
                if (k.src_sel != (both ? 1u : 0u) || k.dst_sel != 0) return "v: selectors";
                if (k.dst_base != im.dst_offset + p * ds * (unsigned long long)im.out_h || k.dst_stride != ds) return "v: destination";
                if (!both && (k.src_base != im.src_offset + p * ss * (unsigned long long)im.h || k.src_stride != ss)) return "v: source";
                if (both && (k.src_base != plan.h.images[hi - 1].dst_base || k.src_stride != plan.h.images[hi - 1].dst_stride)) return "v: not the horizontal pass's output";
                bool vec = true; // by the actual addresses of every row
                for (int row = 0; row < im.h && row < 4; row++) vec &= ((both ? 0 : s.src_addr) + k.src_base + (unsigned long long)row * k.src_stride) % 4 == 0;
                for (int row = 0; row < im.out_h && row < 4; row++) vec &= (s.dst_addr + k.dst_base + (unsigned long long)row * k.dst_stride) % 4 == 0;
                if (k.vec && !vec) return "v: the dword flag set for rows off 4 bytes";
                if (im.h >= 2 && im.out_h >= 2 && (k.vec != 0) != vec) return "v: the dword flag not set";
                if (k.unit0 != vu) return "v: unit0";
                std::vector<unsigned char> seen((size_t)k.lanes * k.n_out, 0);
                for (unsigned long long u = vu; u < vu + k.units; u++) {
                    if (u >= plan.v.map.size() || plan.v.map[(size_t)u] != vi) return "v: map entry";
                    const unsigned ur = (unsigned)(u - k.unit0);
                    const unsigned row = k.groups == 1 ? ur : (unsigned)(((unsigned long long)ur * k.magic) >> 32), seg = ur - row * k.groups;
                    if (row >= k.n_out || seg >= k.groups) return "v: unit position";
                    const hvc::ResizeRecK &rec = plan.recs[k.rec0 + row];
                    if (rec.xmin + rec.count > (unsigned)im.h) return "v: a window beyond the rows";
                    if (rec.count && (size_t)rec.first + (size_t)(rec.count - 1) * k.tap_stride >= plan.taps.size()) return "v: a tap beyond the table";
                    for (unsigned lane = 0; lane < 64; lane++) {
                        const unsigned lr = seg * 64 + lane;
                        if (lr >= k.lanes) continue;
                        if (seen[(size_t)row * k.lanes + lr]++) return "v: a lane twice";
                    }
                }
                for (unsigned char v : seen)
                    if (v != 1) return "v: a lane without a unit";
                vu += k.units;
                vi++;
            }
        }
    }
    if (hi != plan.h.images.size() || vi != plan.v.images.size() || hu != plan.h.map.size() || vu != plan.v.map.size()) return "totals";
    for (size_t a = 0; a < plan.tables.size(); a++)
        for (size_t b = a + 1; b < plan.tables.size(); b++)
            if (plan.tables[a].n_in == plan.tables[b].n_in && plan.tables[a].n_out == plan.tables[b].n_out && plan.tables[a].filter == plan.tables[b].filter)
                return "a table twice";
    return "";
}

void print_pass(const char *name, const hvc::ResizePass &p) {
    for (size_t i = 0; i < p.images.size(); i++) {
        const hvc::ResizeImageK &k = p.images[i];
        std::printf("%s %zu %d %llu %llu %llu %llu %u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", name, i, p.image[i], k.src_base, k.dst_base, k.src_stride,
                    k.dst_stride, k.rec0, k.tap_stride, k.n_out, k.rows, k.ch, k.row_bytes, k.groups, k.magic, k.lanes, k.units, k.unit0, k.src_sel,
                    k.dst_sel, k.vec);
    }
    std::printf("%smap", name);
    for (unsigned u : p.map) std::printf(" %u", u);
    std::printf("\n");
}

int cmd_plan(const char *path) {
    std::vector<unsigned char> raw;
    if (!read_all(path, raw) || raw.size() < 48) return 2;
    long long h[6];
    std::memcpy(h, raw.data(), sizeof h);
    const long long n = h[0], nl = h[1];
    if (n < 0 || raw.size() != sizeof h + (size_t)n * 64 + (nl > 0 ? (size_t)nl * 4 : 0)) return 2;
    Set s;
    s.layout = (int)h[2], s.filter = (int)h[3], s.src_addr = (uintptr_t)h[4], s.dst_addr = (uintptr_t)h[5];
    s.images.resize((size_t)n);
    for (long long i = 0; i < n; i++) {
        long long v[8];
        std::memcpy(v, raw.data() + sizeof h + 64 * (size_t)i, sizeof v);
        hvc::ResizeImage &im = s.images[(size_t)i];
        im.w = (int)v[0], im.h = (int)v[1], im.out_w = (int)v[2], im.out_h = (int)v[3];
        im.src_offset = (size_t)v[4], im.src_row_stride = (size_t)v[5], im.dst_offset = (size_t)v[6], im.dst_row_stride = (size_t)v[7];
    }
    if (nl >= 0) {
        s.has_list = true;
        s.list.resize((size_t)nl);
        if (nl) std::memcpy(s.list.data(), raw.data() + sizeof h + 64 * (size_t)n, (size_t)nl * 4);
        for (int f : s.list)
            if (f < 0 || f >= n) return 2;
    }
    hvc::ResizePlan plan;
    const int r = build(s, plan);
    std::printf("status %d\n", r);
    if (r) {
        std::printf("empty %d\n", (int)(plan.h.images.empty() && plan.v.images.empty() && plan.recs.empty() && plan.taps.empty() && plan.mid_bytes == 0));
        return 0;
    }
    const std::string bad = check_plan(s, plan);
    std::printf("check %s\n", bad.empty() ? "ok" : bad.c_str());
    std::printf("mid %zu\n", plan.mid_bytes);
    std::printf("words %zu %zu\n", plan.recs.size(), plan.taps.size());
    for (const hvc::ResizeTableKey &t : plan.tables) std::printf("table %d %d %d %u\n", t.n_in, t.n_out, t.filter, t.rec0);
    print_pass("h", plan.h);
    print_pass("v", plan.v);
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
    static const int SIDES[] = {1, 2, 3, 7, 8, 9, 21, 63, 64, 65, 84, 85, 86, 100, 255, 256, 257, 340, 342, 480, 1025};
    const unsigned NS = sizeof SIDES / sizeof SIDES[0];
    int refused = 0;
    for (int it = 0; it < count; it++) {
        Set s;
        s.layout = (int)rnd(2), s.filter = (int)rnd(3);
        s.src_addr = (uintptr_t)0x7f0000000000ull + (rnd(3) ? 0 : rnd(8));
        s.dst_addr = (uintptr_t)0x7e0000000000ull + (rnd(3) ? 0 : rnd(8));
        const int n = 1 + (int)rnd(10);
        size_t src = 0, dst = 0;
        for (int f = 0; f < n; f++) {
            hvc::ResizeImage im;
            im.w = SIDES[rnd(NS)], im.h = rnd(3) ? SIDES[rnd(NS)] : 1 + (int)rnd(5);
            im.out_w = rnd(4) ? SIDES[rnd(NS)] : im.w, im.out_h = rnd(4) ? SIDES[rnd(NS)] : im.h;
            const size_t st = hvc::resize_row_bytes(s.layout, im.w), dt = hvc::resize_row_bytes(s.layout, im.out_w);
            im.src_row_stride = rnd(2) ? 0 : (st + rnd(9)) & ~(size_t)(rnd(2) ? 3 : 0);
            if (im.src_row_stride && im.src_row_stride < st) im.src_row_stride = st + 4;
            im.dst_row_stride = rnd(2) ? 0 : (dt + 3 + rnd(9)) & ~(size_t)(rnd(2) ? 3 : 0);
            im.src_offset = src, im.dst_offset = dst;
            src += hvc::resize_span(s.layout, im.w, im.h, im.src_row_stride ? im.src_row_stride : st) + rnd(4);
            dst += hvc::resize_span(s.layout, im.out_w, im.out_h, im.dst_row_stride ? im.dst_row_stride : dt) + rnd(4);
            s.images.push_back(im);
        }
        if (rnd(2)) {
            s.has_list = true;
            for (int f = 0; f < n; f++)
                if (rnd(4)) s.list.push_back(f);
        }
        const bool spoil = rnd(10) == 0;
        if (spoil) s.images[rnd((unsigned)n)].out_w = 0;
        hvc::ResizePlan plan;
        const int r = build(s, plan);
        if (r) {
            bool listed = !s.has_list;
            for (int f : s.list) listed |= s.images[(size_t)f].out_w == 0;
            if (!(spoil && listed && r == HVC_E_INVALID_ARG)) {
                std::printf("set %d: status %d\n", it, r);
                return 1;
            }
            refused++;
            continue;
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
    if (argc >= 5 && !std::strcmp(argv[1], "sweep")) return cmd_sweep(argv[2], argc - 3, argv + 3);
    if (argc >= 3 && !std::strcmp(argv[1], "plan")) return cmd_plan(argv[2]);
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return cmd_random(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 7 && !std::strcmp(argv[1], "status")) {
        std::printf("status %d\n", hvc::resize_image_status(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6])));
        return 0;
    }
    std::fprintf(stderr, "usage: resize_plan_harness sweep OUT N_IN... -- N_OUT... | plan FILE | random SEED COUNT | status W H OUT_W OUT_H FILTER\n");
    return 2;
}
