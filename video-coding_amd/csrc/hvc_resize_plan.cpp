// hvc_resize_plan.cpp -- host plan of the resampling step over a mixed set (hvc_resize_plan.h): the axis tables of the
// definition in include/hvc_jpeg.h (Resizing), the image descriptors and the work map of each pass.  Plain C++ (no HIP),
// usable without a GPU.  Compiled with -ffp-contract=off: every product and every sum of the weights rounds by itself.
#include <cmath>
#include <cstring>
#include <new>

#include "hvc_resize_plan.h"

namespace hvc {
namespace {

double filter_support(int filter) { return filter == HVC_RESIZE_BOX ? 0.5 : filter == HVC_RESIZE_BILINEAR ? 1.0 : 2.0; }

double filter_weight(int filter, double x) {
    switch (filter) {
    case HVC_RESIZE_BOX: return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case HVC_RESIZE_BILINEAR:
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    default: {
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
        if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
        return 0.0;
    }
    }
}

bool known_filter(int filter) { return filter == HVC_RESIZE_BOX || filter == HVC_RESIZE_BILINEAR || filter == HVC_RESIZE_BICUBIC; }

struct AxisGeometry {
    double scale, support, ss, in0;
};
// the window [in0, in1) of the axis: the span is subtracted in SINGLE precision and then widened (Pillow's float box)
AxisGeometry axis_geometry(int n_out, int filter, float in0, float in1) {
    AxisGeometry g;
    const float span = in1 - in0;
    g.scale = (double)span / (double)n_out;
    const double fs = g.scale < 1.0 ? 1.0 : g.scale;
    g.support = filter_support(filter) * fs;
    g.ss = 1.0 / fs;
    g.in0 = (double)in0;
    return g;
}
// the window of output position xx: [xmin, xmax)
void axis_window(const AxisGeometry &g, int n_in, int xx, double &center, int &xmin, int &xmax) {
    center = g.in0 + ((double)xx + 0.5) * g.scale;
    xmin = (int)(center - g.support + 0.5); // (sizes <= 2^24: every value here fits an int)
    if (xmin < 0) xmin = 0;
    xmax = (int)(center + g.support + 0.5);
    if (xmax > n_in) xmax = n_in;
}

// the window itself: finite, inside the samples, a span above 0 in single precision
bool box_ok(int n_in, float in0, float in1) {
    if (!std::isfinite(in0) || !std::isfinite(in1)) return false;
    if (in0 < 0.0f || in1 > (float)n_in) return false;
    const float span = in1 - in0;
    return span > 0.0f;
}

// sizes, filter, the tap bound and the table bound: what can be said before a weight is computed; kmax out
int axis_check(int n_in, int n_out, int filter, float in0, float in1, unsigned &kmax) {
    kmax = 0;
    if (n_in < 1 || n_out < 1 || !known_filter(filter)) return HVC_E_INVALID_ARG;
    if (n_in > (1 << 24) || n_out > (1 << 24)) return HVC_E_TOO_LARGE;
    if (!box_ok(n_in, in0, in1)) return HVC_E_INVALID_ARG;
    const AxisGeometry g = axis_geometry(n_out, filter, in0, in1);
    for (int xx = 0; xx < n_out; xx++) {
        double center;
        int xmin, xmax;
        axis_window(g, n_in, xx, center, xmin, xmax);
        const int count = xmax - xmin;
        if (count < 0) return HVC_E_INTERNAL;
        if ((unsigned)count > kmax) kmax = (unsigned)count;
        if (kmax > HVC_RESIZE_MAX_TAPS) return HVC_E_TOO_LARGE;
    }
    if ((unsigned long long)kmax * (unsigned)n_out > HVC_RESIZE_MAX_TABLE_WORDS) return HVC_E_TOO_LARGE;
    return HVC_OK;
}

uint32_t float_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

} // namespace

int resize_axis_build_box(int n_in, int n_out, int filter, float in0, float in1, bool reversed, unsigned shift,
                          std::vector<ResizeRecK> &recs, std::vector<int> &taps) {
    recs.clear();
    taps.clear();
    unsigned kmax = 0;
    const int r = axis_check(n_in, n_out, filter, in0, in1, kmax);
    if (r) return r;
    const AxisGeometry g = axis_geometry(n_out, filter, in0, in1);
    recs.resize((size_t)n_out);
    taps.assign((size_t)kmax * (size_t)n_out, 0);
    std::vector<double> w(kmax ? kmax : 1);
    for (int xx = 0; xx < n_out; xx++) {
        double center;
        int xmin, xmax;
        axis_window(g, n_in, xx, center, xmin, xmax);
        const int count = xmax - xmin;
        const size_t p = (size_t)(reversed ? n_out - 1 - xx : xx); // where the position's record and taps go
        double ww = 0.0;
        for (int i = 0; i < count; i++) {
            w[(size_t)i] = filter_weight(filter, ((double)(i + xmin) - center + 0.5) * g.ss);
            ww += w[(size_t)i];
        }
        long long abs_sum = 0;
        for (int i = 0; i < count; i++) {
            double v = w[(size_t)i];
            if (ww != 0.0) v /= ww;
            const double s = v * (double)(1 << HVC_RESIZE_PRECISION_BITS);
            if (!(s > -8388608.0 && s < 8388608.0)) return HVC_E_TOO_LARGE; // |k| < 2^23: one 24-bit multiply (and no cast out of range)
            const int k = v < 0.0 ? (int)(s - 0.5) : (int)(s + 0.5);
            taps[(size_t)i * (size_t)n_out + p] = k;
            abs_sum += k < 0 ? -(long long)k : (long long)k;
        }
        // the int32 accumulator: 2^21 + SUM k * sample with samples of 0 .. 255
        if (255 * abs_sum + (1ll << (HVC_RESIZE_PRECISION_BITS - 1)) >= (1ll << 31)) return HVC_E_TOO_LARGE;
        if ((unsigned)xmin < shift) return HVC_E_INTERNAL;
        recs[p].xmin = (unsigned)xmin - shift;
        recs[p].count = (unsigned)count;
        recs[p].first = (unsigned)p;
    }
    return HVC_OK;
}

int resize_axis_build(int n_in, int n_out, int filter, std::vector<ResizeRecK> &recs, std::vector<int> &taps) {
    return resize_axis_build_box(n_in, n_out, filter, 0.0f, (float)n_in, false, 0, recs, taps); // (n_in <= 2^24: exact; beyond, refused)
}

void resize_axis_window(int n_in, int n_out, int filter, float in0, float in1, unsigned &first, unsigned &last) {
    const AxisGeometry g = axis_geometry(n_out, filter, in0, in1);
    double center;
    int xmin, xmax;
    axis_window(g, n_in, 0, center, xmin, xmax);
    first = (unsigned)xmin;
    axis_window(g, n_in, n_out - 1, center, xmin, xmax);
    last = (unsigned)xmax;
}

int resize_image_status(int w, int h, int out_w, int out_h, int filter) {
    return resize_image_status_box(w, h, out_w, out_h, filter, nullptr, 0);
}

int resize_image_status_box(int w, int h, int out_w, int out_h, int filter, const float *box, int mirror) {
    if (w < 1 || h < 1 || out_w < 1 || out_h < 1 || !known_filter(filter)) return HVC_E_INVALID_ARG;
    if (w > (1 << 24) || h > (1 << 24)) return HVC_E_TOO_LARGE; // (before a side becomes a float)
    const float x0 = box ? box[0] : 0.0f, y0 = box ? box[1] : 0.0f, x1 = box ? box[2] : (float)w, y1 = box ? box[3] : (float)h;
    if (!box_ok(w, x0, x1) || !box_ok(h, y0, y1)) return HVC_E_INVALID_ARG;
    std::vector<ResizeRecK> recs;
    std::vector<int> taps;
    const bool skip_h = resize_axis_skipped(w, out_w, x0, x1), skip_v = resize_axis_skipped(h, out_h, y0, y1);
    int r = HVC_OK;
    if (!skip_h) r = resize_axis_build_box(w, out_w, filter, x0, x1, mirror != 0, 0, recs, taps);
    if (!r && !skip_v) r = resize_axis_build_box(h, out_h, filter, y0, y1, false, 0, recs, taps);
    unsigned long long rows = (unsigned)h; // the rows of the horizontal pass: under a box and both axes, the window's
    if (!r && box && !skip_v && (!skip_h || mirror)) {
        unsigned lo, hi;
        resize_axis_window(h, out_h, filter, y0, y1, lo, hi);
        rows = hi - lo;
    }
    if (!r && ((unsigned long long)out_w * rows * (unsigned)out_w >= (1ull << 32))) r = HVC_E_TOO_LARGE; // (the horizontal lanes)
    return r;
}

namespace {

// the table of an axis in the plan: found, or built and appended; rec0 out
int plan_table(ResizePlan &plan, int n_in, int n_out, int filter, float in0, float in1, bool mirrored, unsigned shift, unsigned &rec0) {
    const uint32_t b0 = float_bits(in0), b1 = float_bits(in1);
    for (const ResizeTableKey &t : plan.tables)
        if (t.n_in == n_in && t.n_out == n_out && t.filter == filter && t.in0_bits == b0 && t.in1_bits == b1 && t.mirrored == (int)mirrored &&
            t.shift == shift) {
            rec0 = t.rec0;
            return HVC_OK;
        }
    std::vector<ResizeRecK> recs;
    std::vector<int> taps;
    const int r = resize_axis_build_box(n_in, n_out, filter, in0, in1, mirrored, shift, recs, taps);
    if (r) return r;
    if (plan.taps.size() + taps.size() > HVC_RESIZE_MAX_TABLE_WORDS || plan.recs.size() + recs.size() > HVC_RESIZE_MAX_TABLE_WORDS)
        return HVC_E_TOO_LARGE;
    rec0 = (unsigned)plan.recs.size();
    const unsigned tap0 = (unsigned)plan.taps.size();
    for (ResizeRecK &k : recs) k.first += tap0;
    plan.recs.insert(plan.recs.end(), recs.begin(), recs.end());
    plan.taps.insert(plan.taps.end(), taps.begin(), taps.end());
    ResizeTableKey key{n_in, n_out, filter, rec0};
    key.in0_bits = b0, key.in1_bits = b1, key.mirrored = (int)mirrored, key.shift = shift;
    plan.tables.push_back(key);
    return HVC_OK;
}

unsigned magic_of(unsigned groups) { return groups == 1 ? 0u : (unsigned)(((1ull << 32) + groups - 1) / groups); }

int add_units(ResizePass &pass, ResizeImageK &k, unsigned long long units, int image) {
    if (pass.map.size() + units > HVC_MIXED_MAX_UNITS) return HVC_E_TOO_LARGE;
    k.units = (unsigned)units;
    k.unit0 = (unsigned)pass.map.size();
    pass.map.insert(pass.map.end(), (size_t)units, (unsigned)pass.images.size());
    pass.images.push_back(k);
    pass.image.push_back(image);
    return HVC_OK;
}

int build(const ResizeImage *images, const int *list, int n_list, int layout, int filter, uintptr_t src_addr, uintptr_t dst_addr,
          const ResizePlanOpts &opts, ResizePlan &plan) {
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (!known_filter(filter)) return HVC_E_INVALID_ARG;
    if (opts.out_elem != 0 && opts.out_elem != 2 && opts.out_elem != 4) return HVC_E_INVALID_ARG;
    if (n_list < 0 || (n_list > 0 && !images)) return HVC_E_INVALID_ARG;
    const unsigned ch = layout == HVC_RGB_PLANAR ? 1 : 3, planes = layout == HVC_RGB_PLANAR ? 3 : 1;
    const bool typed = opts.out_elem != 0;
    const unsigned elem = typed ? (unsigned)opts.out_elem : 1;
    plan.out_elem = opts.out_elem;
    for (int l = 0; l < n_list; l++) {
        const int f = list ? list[l] : l;
        if (f < 0) return HVC_E_INVALID_ARG;
        const ResizeImage &im = images[f];
        if (im.w < 1 || im.h < 1 || im.out_w < 1 || im.out_h < 1) return HVC_E_INVALID_ARG;
        if (im.w > (1 << 24) || im.h > (1 << 24) || im.out_w > (1 << 24) || im.out_h > (1 << 24)) return HVC_E_TOO_LARGE;
        const size_t src_tight = resize_row_bytes(layout, im.w), row8 = resize_row_bytes(layout, im.out_w), dst_tight = row8 * elem;
        const unsigned long long ss = im.src_row_stride ? im.src_row_stride : src_tight, ds = im.dst_row_stride ? im.dst_row_stride : dst_tight;
        if (ss < src_tight || ds < dst_tight) return HVC_E_INVALID_ARG;
        if (ss >= (1ull << 32) || ds >= (1ull << 32)) return HVC_E_TOO_LARGE;
        const float *box = opts.boxes ? opts.boxes + 4 * (size_t)f : nullptr;
        const float x0 = box ? box[0] : 0.0f, y0 = box ? box[1] : 0.0f, x1 = box ? box[2] : (float)im.w, y1 = box ? box[3] : (float)im.h;
        if (!box_ok(im.w, x0, x1) || !box_ok(im.h, y0, y1)) return HVC_E_INVALID_ARG;
        const bool mirrored = opts.mirror && opts.mirror[f];
        const bool skip_h = resize_axis_skipped(im.w, im.out_w, x0, x1), skip_v = resize_axis_skipped(im.h, im.out_h, y0, y1);
        // neither axis: the copy, through the vertical pass; a mirror runs the horizontal axis, a typed output the vertical one
        const bool need_h = !skip_h || mirrored, need_v = !skip_v || !need_h || typed;
        const bool both = need_h && need_v;
        // a skipped axis that runs all the same takes the identity table: box n -> n, one tap of 2^22 per position
        const int filter_h = skip_h ? (int)HVC_RESIZE_BOX : filter, filter_v = skip_v ? (int)HVC_RESIZE_BOX : filter;
        // the source rows the vertical axis reads: [y_lo, y_hi)
        unsigned y_lo = 0, y_hi = (unsigned)im.h;
        if (need_v) resize_axis_window(im.h, im.out_h, filter_v, y0, y1, y_lo, y_hi);
        if (y_hi <= y_lo || y_hi > (unsigned)im.h) return HVC_E_INTERNAL;
        // both axes: the horizontal pass covers only those rows, and the intermediate holds only them: out_w x (y_hi - y_lo),
        // rows on 4 bytes, the image (every plane) on 64
        const unsigned long long rows_h = both ? y_hi - y_lo : (unsigned)im.h, row0_h = both ? y_lo : 0;
        const unsigned long long ms = (row8 + 3) & ~(unsigned long long)3;
        unsigned long long mid0 = 0;
        if (both) {
            mid0 = ((unsigned long long)plan.mid_bytes + 63) & ~(unsigned long long)63;
            plan.mid_bytes = (size_t)(mid0 + ms * rows_h * planes);
        }
        unsigned rec_h = 0, rec_v = 0;
        int r;
        if (need_h && (r = plan_table(plan, im.w, im.out_w, filter_h, x0, x1, mirrored, 0, rec_h))) return r;
        if (need_v && (r = plan_table(plan, im.h, im.out_h, filter_v, y0, y1, false, y_lo, rec_v))) return r;
        for (unsigned p = 0; p < planes; p++) {
            if (need_h) {
                ResizeImageK k;
                std::memset(&k, 0, sizeof k);
                k.src_base = (unsigned long long)im.src_offset + p * ss * (unsigned long long)im.h + row0_h * ss;
                k.src_stride = ss;
                k.dst_sel = both ? 1 : 0;
                k.dst_base = both ? mid0 + p * ms * rows_h : (unsigned long long)im.dst_offset + p * ds * (unsigned long long)im.out_h;
                k.dst_stride = both ? ms : ds;
                k.rec0 = rec_h, k.tap_stride = (unsigned)im.out_w;
                k.n_out = (unsigned)im.out_w, k.rows = (unsigned)rows_h, k.ch = ch;
                k.row_bytes = (unsigned)row8;
                k.groups = (unsigned)im.out_w, k.magic = magic_of(k.groups);
                const unsigned long long lanes = (unsigned long long)im.out_w * rows_h;
                // row = umulhi(t, magic) is exact for t * groups < 2^32
                if (lanes * k.groups >= (1ull << 32)) return HVC_E_TOO_LARGE;
                k.lanes = (unsigned)lanes;
                if ((r = add_units(plan.h, k, (lanes + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT, f))) return r;
            }
            if (need_v) {
                ResizeImageK k;
                std::memset(&k, 0, sizeof k);
                // (the table is shifted by y_lo: the source starts at that row)
                k.src_sel = both ? 1 : 0;
                k.src_base = both ? mid0 + p * ms * rows_h : (unsigned long long)im.src_offset + p * ss * (unsigned long long)im.h + y_lo * ss;
                k.src_stride = both ? ms : ss;
                k.dst_base = (unsigned long long)im.dst_offset + p * ds * (unsigned long long)im.out_h;
                k.dst_stride = ds;
                k.rec0 = rec_v, k.tap_stride = (unsigned)im.out_h;
                k.n_out = (unsigned)im.out_h, k.rows = both ? (unsigned)rows_h : (unsigned)im.h - y_lo, k.ch = ch; // (rows: those from src_base on)
                k.row_bytes = (unsigned)row8;
                k.lanes = (k.row_bytes + 3) / 4;
                k.groups = (k.lanes + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT, k.magic = magic_of(k.groups);
                const unsigned long long units = (unsigned long long)k.groups * (unsigned)im.out_h;
                if (units * k.groups >= (1ull << 32)) return HVC_E_TOO_LARGE; // (row = umulhi(u, magic), as above)
                const unsigned long long sa = both ? 0 : (unsigned long long)src_addr;
                if (!typed) {
                    k.vec = ((sa + k.src_base) | k.src_stride | ((unsigned long long)dst_addr + k.dst_base) | k.dst_stride) % 4 == 0;
                } else { // the source's dword loads and the destination's 8- / 16-byte stores are judged apart
                    k.vec = ((sa + k.src_base) | k.src_stride) % 4 == 0;
                    k.dvec = (((unsigned long long)dst_addr + k.dst_base) | k.dst_stride) % (4 * elem) == 0;
                    k.chan = layout == HVC_RGB_PLANAR ? p : 3;
                }
                if ((r = add_units(plan.v, k, units, f))) return r;
            }
        }
    }
    return HVC_OK;
}

} // namespace

int resize_plan_build(const ResizeImage *images, const int *list, int n_list, int layout, int filter, uintptr_t src_addr,
                      uintptr_t dst_addr, ResizePlan &plan) {
    return resize_plan_build_opts(images, list, n_list, layout, filter, src_addr, dst_addr, ResizePlanOpts(), plan);
}

int resize_plan_build_opts(const ResizeImage *images, const int *list, int n_list, int layout, int filter, uintptr_t src_addr,
                           uintptr_t dst_addr, const ResizePlanOpts &opts, ResizePlan &plan) {
    plan.clear();
    const int r = build(images, list, n_list, layout, filter, src_addr, dst_addr, opts, plan);
    if (r) plan.clear();
    return r;
}

} // namespace hvc
