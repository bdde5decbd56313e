// Stand-alone driver of the box / mirror / typed forms of csrc/hvc_resize_plan.cpp for tests/test_resize_box_plan.py, built by
// Makefile.resize_box with -fsanitize=address,undefined and -ffp-contract=off (CPU only, no device code):
//   resize_box_plan_harness axes IN OUT     IN = int32 records of 7: n_in, n_out, filter, bits of in0, bits of in1, reversed, shift;
//                                           OUT receives, per axis, int32 status, kmax, then (status 0) xmin[n_out], count[n_out],
//                                           first[n_out], taps[kmax * n_out] as hvc::resize_axis_build_box stores them
//   resize_box_plan_harness plan FILE OUT   FILE = int64 n_images, n_list (-1: no list), layout, filter, src_addr, dst_addr,
//                                           has_boxes, has_mirror, out_elem; per image int64 w, h, out_w, out_h, src_offset,
//                                           src_row_stride, dst_offset, dst_row_stride, mirror and 4 x float32 box (8 bytes of
//                                           padding behind); int32 list[n_list].  Prints the plan hvc::resize_plan_build_opts
//                                           makes and what check_plan says of it; OUT receives int32 n_recs, n_taps, the records
//                                           (xmin, count, first) and the taps
//   resize_box_plan_harness random SEED COUNT   COUNT seeded random sets with boxes, mirrors and typed outputs, each held
//                                           against check_plan here: every access stays inside its image or intermediate
//   resize_box_plan_harness status W H OUT_W OUT_H FILTER MIRROR [X0 Y0 X1 Y1 as bits]   hvc::resize_image_status_box
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

float float_of(unsigned bits) {
    float v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
}

int cmd_axes(const char *in_path, const char *out_path) {
    std::vector<unsigned char> raw;
    if (!read_all(in_path, raw) || raw.size() % 28) return 2;
    FILE *f = std::fopen(out_path, "wb");
    if (!f) return 2;
    for (size_t at = 0; at < raw.size(); at += 28) {
        int a[7];
        std::memcpy(a, raw.data() + at, sizeof a);
        std::vector<hvc::ResizeRecK> recs;
        std::vector<int> taps;
        const int r = hvc::resize_axis_build_box(a[0], a[1], a[2], float_of((unsigned)a[3]), float_of((unsigned)a[4]), a[5] != 0, (unsigned)a[6], recs, taps);
        const int n_out = a[1];
        const int head[2] = {r, r || n_out < 1 ? 0 : (int)(taps.size() / (size_t)n_out)};
        std::fwrite(head, sizeof head, 1, f);
        if (r) continue;
        std::vector<int> col((size_t)n_out);
        for (int p = 0; p < n_out; p++) col[(size_t)p] = (int)recs[(size_t)p].xmin;
        std::fwrite(col.data(), 4, col.size(), f);
        for (int p = 0; p < n_out; p++) col[(size_t)p] = (int)recs[(size_t)p].count;
        std::fwrite(col.data(), 4, col.size(), f);
        for (int p = 0; p < n_out; p++) col[(size_t)p] = (int)recs[(size_t)p].first;
        std::fwrite(col.data(), 4, col.size(), f);
        if (!taps.empty()) std::fwrite(taps.data(), 4, taps.size(), f);
    }
    std::fclose(f);
    std::printf("ok %zu\n", raw.size() / 28);
    return 0;
}

struct Set {
    std::vector<hvc::ResizeImage> images;
    std::vector<float> boxes;
    std::vector<uint8_t> mirror;
    std::vector<int> list;
    bool has_list = false, has_boxes = false, has_mirror = false;
    int layout = 0, filter = 0, out_elem = 0;
    uintptr_t src_addr = 0, dst_addr = 0;
};

int build(const Set &s, hvc::ResizePlan &plan) {
    hvc::ResizePlanOpts o;
    o.boxes = s.has_boxes ? s.boxes.data() : nullptr;
    o.mirror = s.has_mirror ? s.mirror.data() : nullptr;
    o.out_elem = s.out_elem;
    return hvc::resize_plan_build_opts(s.images.data(), s.has_list ? s.list.data() : nullptr, s.has_list ? (int)s.list.size() : (int)s.images.size(),
                                       s.layout, s.filter, s.src_addr, s.dst_addr, o, plan);
}

// What every plan must have, whatever the options; returns an empty string or what is wrong.  It does not compute a weight:
// the tables are held against the numpy form by the test.  Here: every image has the descriptors its axes ask for, every lane
// of every pass lies in exactly one (unit, lane), and every read and write stays inside its image, its record or the
// intermediate.
std::string check_plan(const Set &s, const hvc::ResizePlan &plan) {
    const int n_list = s.has_list ? (int)s.list.size() : (int)s.images.size();
    const unsigned planes = s.layout == HVC_RGB_PLANAR ? 3 : 1, ch = s.layout == HVC_RGB_PLANAR ? 1 : 3;
    const unsigned elem = s.out_elem ? (unsigned)s.out_elem : 1;
    if (plan.out_elem != s.out_elem) return "out_elem";
    size_t hi = 0, vi = 0;
    unsigned long long hu = 0, vu = 0;
    for (int l = 0; l < n_list; l++) {
        const int f = s.has_list ? s.list[(size_t)l] : l;
        const hvc::ResizeImage &im = s.images[(size_t)f];
        const float *b = s.has_boxes ? &s.boxes[4 * (size_t)f] : nullptr;
        const float x0 = b ? b[0] : 0.0f, y0 = b ? b[1] : 0.0f, x1 = b ? b[2] : (float)im.w, y1 = b ? b[3] : (float)im.h;
        const bool mirrored = s.has_mirror && s.mirror[(size_t)f];
        const bool skip_h = im.out_w == im.w && x0 == 0.0f && x1 == (float)im.w, skip_v = im.out_h == im.h && y0 == 0.0f && y1 == (float)im.h;
        const bool need_h = !skip_h || mirrored, need_v = !skip_v || !need_h || s.out_elem != 0, both = need_h && need_v;
        const unsigned long long st = hvc::resize_row_bytes(s.layout, im.w), row8 = hvc::resize_row_bytes(s.layout, im.out_w), dt = row8 * elem;
        const unsigned long long ss = im.src_row_stride ? im.src_row_stride : st, ds = im.dst_row_stride ? im.dst_row_stride : dt;
        for (unsigned p = 0; p < planes; p++) {
            const unsigned long long plane0 = im.src_offset + p * ss * (unsigned long long)im.h; // the plane's first source byte
            unsigned long long h_rows = 0, h_dst = 0, h_stride = 0;
            if (need_h) {
                if (hi >= plan.h.images.size()) return "an image without a horizontal descriptor";
                const hvc::ResizeImageK &k = plan.h.images[hi];
                if (plan.h.image[hi] != f) return "h: image index";
                if (k.ch != ch || k.n_out != (unsigned)im.out_w || k.groups != (unsigned)im.out_w || k.tap_stride != (unsigned)im.out_w) return "h: geometry";
                if (k.lanes != (unsigned long long)im.out_w * k.rows) return "h: lanes";
                if (k.src_sel != 0 || k.dst_sel != (both ? 1u : 0u) || k.src_stride != ss) return "h: selectors";
                // the source rows: whole rows of the plane, inside it
                if (k.src_base < plane0 || (k.src_base - plane0) % ss) return "h: the first source row";
                const unsigned long long r0 = (k.src_base - plane0) / ss;
                if (k.rows < 1 || r0 + k.rows > (unsigned long long)im.h) return "h: rows beyond the image";
                if (!both && (r0 != 0 || k.rows != (unsigned)im.h)) return "h: a window without a vertical pass";
                if (!both && (k.dst_base != im.dst_offset + p * ds * (unsigned long long)im.out_h || k.dst_stride != ds)) return "h: destination";
                if (both && (k.dst_base % 64 != 0 && p == 0)) return "h: intermediate off 64 bytes";
                if (both && (k.dst_stride % 4 != 0 || k.dst_stride < row8 || k.dst_base + k.dst_stride * (unsigned long long)k.rows > plan.mid_bytes)) return "h: intermediate";
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
                        if (k.rec0 + xx >= plan.recs.size()) return "h: a record beyond the tables";
                        const hvc::ResizeRecK &rec = plan.recs[k.rec0 + xx];
                        if (rec.xmin + rec.count > (unsigned)im.w) return "h: a window beyond the row";
                        if (rec.count && (size_t)rec.first + (size_t)(rec.count - 1) * k.tap_stride >= plan.taps.size()) return "h: a tap beyond the table";
                    }
                }
                for (unsigned char v : seen)
                    if (v != 1) return "h: a lane without a unit";
                h_rows = k.rows, h_dst = k.dst_base, h_stride = k.dst_stride;
                hu += k.units;
                hi++;
            }
            if (need_v) {
                if (vi >= plan.v.images.size()) return "an image without a vertical descriptor";
                const hvc::ResizeImageK &k = plan.v.images[vi];
                if (plan.v.image[vi] != f) return "v: image index";
                if (k.n_out != (unsigned)im.out_h || k.row_bytes != row8 || k.tap_stride != (unsigned)im.out_h) return "v: geometry";
                if (k.lanes != (k.row_bytes + 3) / 4 || k.groups != (k.lanes + 63) / 64 || k.units != k.groups * k.n_out) return "v: lanes";
                if (k.src_sel != (both ? 1u : 0u) || k.dst_sel != 0) return "v: selectors";
                if (k.dst_base != im.dst_offset + p * ds * (unsigned long long)im.out_h || k.dst_stride != ds) return "v: destination";
                if (both) { // it reads exactly what the horizontal pass wrote
                    if (k.src_base != h_dst || k.src_stride != h_stride || k.rows != h_rows) return "v: not the horizontal pass's output";
                } else {
                    if (k.src_stride != ss || k.src_base < plane0 || (k.src_base - plane0) % ss) return "v: source";
                    if ((k.src_base - plane0) / ss + k.rows != (unsigned long long)im.h) return "v: rows beyond the image";
                }
                bool vec = true, dvec = true; // by the actual addresses of every row
                for (unsigned row = 0; row < k.rows && row < 4; row++) vec &= ((both ? 0 : s.src_addr) + k.src_base + (unsigned long long)row * k.src_stride) % 4 == 0;
                for (int row = 0; row < im.out_h && row < 4; row++) {
                    const unsigned long long a = s.dst_addr + k.dst_base + (unsigned long long)row * k.dst_stride;
                    if (s.out_elem) dvec &= a % (4 * elem) == 0;
                    else vec &= a % 4 == 0;
                }
                if (k.vec && !vec) return "v: the dword flag set for rows off 4 bytes";
                if (k.rows >= 2 && im.out_h >= 2 && (k.vec != 0) != vec) return "v: the dword flag not set";
                if (!s.out_elem && (k.dvec || k.chan)) return "v: typed fields without a typed output";
                if (s.out_elem) {
                    if (k.dvec && !dvec) return "v: the wide-store flag set for rows off 4 elements";
                    if (im.out_h >= 2 && (k.dvec != 0) != dvec) return "v: the wide-store flag not set";
                    if (k.chan != (s.layout == HVC_RGB_PLANAR ? p : 3u)) return "v: channel";
                }
                if (k.unit0 != vu) return "v: unit0";
                std::vector<unsigned char> seen((size_t)k.lanes * k.n_out, 0);
                for (unsigned long long u = vu; u < vu + k.units; u++) {
                    if (u >= plan.v.map.size() || plan.v.map[(size_t)u] != vi) return "v: map entry";
                    const unsigned ur = (unsigned)(u - k.unit0);
                    const unsigned row = k.groups == 1 ? ur : (unsigned)(((unsigned long long)ur * k.magic) >> 32), seg = ur - row * k.groups;
                    if (row >= k.n_out || seg >= k.groups) return "v: unit position";
                    if (k.rec0 + row >= plan.recs.size()) return "v: a record beyond the tables";
                    const hvc::ResizeRecK &rec = plan.recs[k.rec0 + row];
                    if (rec.xmin + rec.count > k.rows) return "v: a window beyond the rows";
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
        for (size_t b = a + 1; b < plan.tables.size(); b++) {
            const hvc::ResizeTableKey &x = plan.tables[a], &y = plan.tables[b];
            if (x.n_in == y.n_in && x.n_out == y.n_out && x.filter == y.filter && x.in0_bits == y.in0_bits && x.in1_bits == y.in1_bits &&
                x.mirrored == y.mirrored && x.shift == y.shift)
                return "a table twice";
        }
    return "";
}

void print_pass(const char *name, const hvc::ResizePass &p) {
    for (size_t i = 0; i < p.images.size(); i++) {
        const hvc::ResizeImageK &k = p.images[i];
        std::printf("%s %zu %d %llu %llu %llu %llu %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", name, i, p.image[i], k.src_base, k.dst_base,
                    k.src_stride, k.dst_stride, k.rec0, k.tap_stride, k.n_out, k.rows, k.ch, k.row_bytes, k.groups, k.magic, k.lanes, k.units, k.unit0,
                    k.src_sel, k.dst_sel, k.vec, k.dvec, k.chan);
    }
    std::printf("%smap", name);
    for (unsigned u : p.map) std::printf(" %u", u);
    std::printf("\n");
}

const size_t IMAGE_BYTES = 9 * 8 + 4 * 4 + 8;

int cmd_plan(const char *path, const char *out_path) {
    std::vector<unsigned char> raw;
    if (!read_all(path, raw) || raw.size() < 72) return 2;
    long long h[9];
    std::memcpy(h, raw.data(), sizeof h);
    const long long n = h[0], nl = h[1];
    if (n < 0 || raw.size() != sizeof h + (size_t)n * IMAGE_BYTES + (nl > 0 ? (size_t)nl * 4 : 0)) return 2;
    Set s;
    s.layout = (int)h[2], s.filter = (int)h[3], s.src_addr = (uintptr_t)h[4], s.dst_addr = (uintptr_t)h[5];
    s.has_boxes = h[6] != 0, s.has_mirror = h[7] != 0, s.out_elem = (int)h[8];
    s.images.resize((size_t)n);
    s.boxes.resize(4 * (size_t)n + 4);
    s.mirror.resize((size_t)n + 1);
    for (long long i = 0; i < n; i++) {
        const unsigned char *at = raw.data() + sizeof h + IMAGE_BYTES * (size_t)i;
        long long v[9];
        std::memcpy(v, at, sizeof v);
        hvc::ResizeImage &im = s.images[(size_t)i];
        im.w = (int)v[0], im.h = (int)v[1], im.out_w = (int)v[2], im.out_h = (int)v[3];
        im.src_offset = (size_t)v[4], im.src_row_stride = (size_t)v[5], im.dst_offset = (size_t)v[6], im.dst_row_stride = (size_t)v[7];
        s.mirror[(size_t)i] = (uint8_t)(v[8] != 0);
        std::memcpy(&s.boxes[4 * (size_t)i], at + sizeof v, 16);
    }
    if (nl >= 0) {
        s.has_list = true;
        s.list.resize((size_t)nl);
        if (nl) std::memcpy(s.list.data(), raw.data() + sizeof h + IMAGE_BYTES * (size_t)n, (size_t)nl * 4);
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
    for (const hvc::ResizeTableKey &t : plan.tables)
        std::printf("table %d %d %d %u %u %u %d %u\n", t.n_in, t.n_out, t.filter, t.rec0, t.in0_bits, t.in1_bits, t.mirrored, t.shift);
    print_pass("h", plan.h);
    print_pass("v", plan.v);
    FILE *f = std::fopen(out_path, "wb");
    if (!f) return 2;
    const int head[2] = {(int)plan.recs.size(), (int)plan.taps.size()};
    std::fwrite(head, sizeof head, 1, f);
    if (!plan.recs.empty()) std::fwrite(plan.recs.data(), sizeof(hvc::ResizeRecK), plan.recs.size(), f);
    if (!plan.taps.empty()) std::fwrite(plan.taps.data(), 4, plan.taps.size(), f);
    std::fclose(f);
    return 0;
}

unsigned long long rng_state;
unsigned rnd(unsigned n) { // splitmix64
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) % n);
}
float frac(unsigned n) { return (float)rnd(n * 64) / 64.0f; } // a value of 0 .. n in steps of 1 / 64

int cmd_random(unsigned long long seed, int count) {
    rng_state = seed;
    static const int SIDES[] = {1, 2, 3, 7, 8, 9, 21, 63, 64, 65, 84, 85, 86, 100, 255, 256, 257, 340, 342, 480};
    const unsigned NS = sizeof SIDES / sizeof SIDES[0];
    int refused = 0;
    for (int it = 0; it < count; it++) {
        Set s;
        s.layout = (int)rnd(2), s.filter = (int)rnd(3);
        static const int ELEMS[] = {0, 0, 2, 4};
        s.out_elem = ELEMS[rnd(4)];
        s.has_boxes = rnd(4) != 0, s.has_mirror = rnd(2) != 0;
        s.src_addr = (uintptr_t)0x7f0000000000ull + (rnd(3) ? 0 : rnd(8));
        s.dst_addr = (uintptr_t)0x7e0000000000ull + (rnd(3) ? 0 : rnd(16) * (s.out_elem ? (unsigned)s.out_elem : 1));
        const unsigned elem = s.out_elem ? (unsigned)s.out_elem : 1;
        const int n = 1 + (int)rnd(8);
        size_t src = 0, dst = 0;
        bool spoiled = false;
        for (int f = 0; f < n; f++) {
            hvc::ResizeImage im;
            im.w = SIDES[rnd(NS)], im.h = rnd(3) ? SIDES[rnd(NS)] : 1 + (int)rnd(5);
            im.out_w = rnd(4) ? SIDES[rnd(NS)] : im.w, im.out_h = rnd(4) ? SIDES[rnd(NS)] : im.h;
            const size_t st = hvc::resize_row_bytes(s.layout, im.w), dt = hvc::resize_row_bytes(s.layout, im.out_w) * elem;
            im.src_row_stride = rnd(2) ? 0 : (st + rnd(9)) & ~(size_t)(rnd(2) ? 3 : 0);
            if (im.src_row_stride && im.src_row_stride < st) im.src_row_stride = st + 4;
            im.dst_row_stride = rnd(2) ? 0 : (dt + 4 * elem + rnd(9) * elem) & ~(size_t)(rnd(2) ? 4 * elem - 1 : 0);
            im.src_offset = src, im.dst_offset = dst;
            src += hvc::resize_span(s.layout, im.w, im.h, im.src_row_stride ? im.src_row_stride : st) + rnd(4);
            dst += (hvc::resize_rows(s.layout, im.out_h) - 1) * (im.dst_row_stride ? im.dst_row_stride : dt) + dt + rnd(4) * elem;
            s.images.push_back(im);
            // the box: whole, integer, fractional, thinner than a pixel, or touching an edge
            float x0 = 0, y0 = 0, x1 = (float)im.w, y1 = (float)im.h;
            switch (rnd(5)) {
            case 0: break;
            case 1: x0 = (float)rnd((unsigned)im.w), x1 = x0 + 1 + (float)rnd((unsigned)(im.w - (int)x0)), y0 = (float)rnd((unsigned)im.h), y1 = y0 + 1 + (float)rnd((unsigned)(im.h - (int)y0)); break;
            case 2: x0 = frac((unsigned)im.w) * 0.5f, x1 = x0 + (float)im.w * 0.5f, y0 = frac((unsigned)im.h) * 0.5f, y1 = y0 + (float)im.h * 0.5f; break;
            case 3: x0 = frac((unsigned)im.w) * 0.5f, x1 = x0 + 0.25f, y0 = frac((unsigned)im.h) * 0.5f, y1 = y0 + 0.125f; break;
            default: x0 = 0, x1 = (float)im.w - frac(1) * 0.5f, y1 = (float)im.h, y0 = frac((unsigned)im.h) * 0.5f; break;
            }
            if (rnd(40) == 0) x1 = x0, spoiled = true; // an empty box: the set is refused if the image is listed
            const float b[4] = {x0, y0, x1, y1};
            s.boxes.insert(s.boxes.end(), b, b + 4);
            s.mirror.push_back((uint8_t)(rnd(3) == 0));
        }
        if (rnd(2)) {
            s.has_list = true;
            for (int f = 0; f < n; f++)
                if (rnd(4)) s.list.push_back(f);
        }
        hvc::ResizePlan plan;
        const int r = build(s, plan);
        if (r) {
            // (sides of at most 480: no bound is met) only the empty box refuses a set, and a refused set leaves an empty plan
            if (!(r == HVC_E_INVALID_ARG && spoiled && s.has_boxes) || !plan.h.images.empty() || !plan.v.images.empty() || plan.mid_bytes) {
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
    if (argc >= 4 && !std::strcmp(argv[1], "axes")) return cmd_axes(argv[2], argv[3]);
    if (argc >= 4 && !std::strcmp(argv[1], "plan")) return cmd_plan(argv[2], argv[3]);
    if (argc >= 4 && !std::strcmp(argv[1], "random")) return cmd_random(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
    if (argc >= 8 && !std::strcmp(argv[1], "status")) {
        float box[4];
        const bool has = argc >= 12;
        for (int i = 0; has && i < 4; i++) box[i] = float_of((unsigned)std::strtoul(argv[8 + i], nullptr, 10));
        std::printf("status %d\n", hvc::resize_image_status_box(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]),
                                                                has ? box : nullptr, std::atoi(argv[7])));
        return 0;
    }
    std::fprintf(stderr, "usage: resize_box_plan_harness axes IN OUT | plan FILE OUT | random SEED COUNT | status W H OUT_W OUT_H FILTER MIRROR [X0 Y0 X1 Y1]\n");
    return 2;
}
