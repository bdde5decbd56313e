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
    double scale, support, ss;
};
AxisGeometry axis_geometry(int n_in, int n_out, int filter) {
    AxisGeometry g;
    g.scale = (double)n_in / (double)n_out;
    const double fs = g.scale < 1.0 ? 1.0 : g.scale;
    g.support = filter_support(filter) * fs;
    g.ss = 1.0 / fs;
    return g;
}
// the window of output position xx: [xmin, xmax)
void axis_window(const AxisGeometry &g, int n_in, int xx, double &center, int &xmin, int &xmax) {
    center = ((double)xx + 0.5) * g.scale;
    xmin = (int)(center - g.support + 0.5); // (sizes <= 2^24: every value here fits an int)
    if (xmin < 0) xmin = 0;
    xmax = (int)(center + g.support + 0.5);
    if (xmax > n_in) xmax = n_in;
}

// sizes, filter, the tap bound and the table bound: what can be said before a weight is computed; kmax out
int axis_check(int n_in, int n_out, int filter, unsigned &kmax) {
    kmax = 0;
    if (n_in < 1 || n_out < 1 || !known_filter(filter)) return HVC_E_INVALID_ARG;
    if (n_in > (1 << 24) || n_out > (1 << 24)) return HVC_E_TOO_LARGE;
    const AxisGeometry g = axis_geometry(n_in, n_out, filter);
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

} // namespace

int resize_axis_build(int n_in, int n_out, int filter, std::vector<ResizeRecK> &recs, std::vector<int> &taps) {
    recs.clear();
    taps.clear();
    unsigned kmax = 0;
    const int r = axis_check(n_in, n_out, filter, kmax);
    if (r) return r;
    const AxisGeometry g = axis_geometry(n_in, n_out, filter);
    recs.resize((size_t)n_out);
    taps.assign((size_t)kmax * (size_t)n_out, 0);
    std::vector<double> w(kmax ? kmax : 1);
    for (int xx = 0; xx < n_out; xx++) {
        double center;
        int xmin, xmax;
        axis_window(g, n_in, xx, center, xmin, xmax);
        const int count = xmax - xmin;
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
            taps[(size_t)i * (size_t)n_out + (size_t)xx] = k;
            abs_sum += k < 0 ? -(long long)k : (long long)k;
        }
        // the int32 accumulator: 2^21 + SUM k * sample with samples of 0 .. 255
        if (255 * abs_sum + (1ll << (HVC_RESIZE_PRECISION_BITS - 1)) >= (1ll << 31)) return HVC_E_TOO_LARGE;
        recs[(size_t)xx].xmin = (unsigned)xmin;
        recs[(size_t)xx].count = (unsigned)count;
        recs[(size_t)xx].first = (unsigned)xx;
    }
    return HVC_OK;
}

int resize_image_status(int w, int h, int out_w, int out_h, int filter) {
    if (w < 1 || h < 1 || out_w < 1 || out_h < 1 || !known_filter(filter)) return HVC_E_INVALID_ARG;
    std::vector<ResizeRecK> recs;
    std::vector<int> taps;
    int r = HVC_OK;
    if (out_w != w) r = resize_axis_build(w, out_w, filter, recs, taps);
    if (!r && out_h != h) r = resize_axis_build(h, out_h, filter, recs, taps);
    if (!r && ((unsigned long long)out_w * (unsigned)h * (unsigned)out_w >= (1ull << 32))) r = HVC_E_TOO_LARGE; // (the horizontal lanes)
    return r;
}

namespace {

// the table of an axis in the plan: found, or built and appended; rec0 out
int plan_table(ResizePlan &plan, int n_in, int n_out, int filter, unsigned &rec0) {
    for (const ResizeTableKey &t : plan.tables)
        if (t.n_in == n_in && t.n_out == n_out && t.filter == filter) {
            rec0 = t.rec0;
            return HVC_OK;
        }
    std::vector<ResizeRecK> recs;
    std::vector<int> taps;
    const int r = resize_axis_build(n_in, n_out, filter, recs, taps);
    if (r) return r;
    if (plan.taps.size() + taps.size() > HVC_RESIZE_MAX_TABLE_WORDS || plan.recs.size() + recs.size() > HVC_RESIZE_MAX_TABLE_WORDS)
        return HVC_E_TOO_LARGE;
    rec0 = (unsigned)plan.recs.size();
    const unsigned tap0 = (unsigned)plan.taps.size();
    for (ResizeRecK &k : recs) k.first += tap0;
    plan.recs.insert(plan.recs.end(), recs.begin(), recs.end());
    plan.taps.insert(plan.taps.end(), taps.begin(), taps.end());
    plan.tables.push_back(ResizeTableKey{n_in, n_out, filter, rec0});
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
          ResizePlan &plan) {
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return HVC_E_INVALID_ARG;
    if (!known_filter(filter)) return HVC_E_INVALID_ARG;
    if (n_list < 0 || (n_list > 0 && !images)) return HVC_E_INVALID_ARG;
    const unsigned ch = layout == HVC_RGB_PLANAR ? 1 : 3, planes = layout == HVC_RGB_PLANAR ? 3 : 1;
    for (int l = 0; l < n_list; l++) {
        const int f = list ? list[l] : l;
        if (f < 0) return HVC_E_INVALID_ARG;
        const ResizeImage &im = images[f];
        if (im.w < 1 || im.h < 1 || im.out_w < 1 || im.out_h < 1) return HVC_E_INVALID_ARG;
        if (im.w > (1 << 24) || im.h > (1 << 24) || im.out_w > (1 << 24) || im.out_h > (1 << 24)) return HVC_E_TOO_LARGE;
        const size_t src_tight = resize_row_bytes(layout, im.w), dst_tight = resize_row_bytes(layout, im.out_w);
        const unsigned long long ss = im.src_row_stride ? im.src_row_stride : src_tight, ds = im.dst_row_stride ? im.dst_row_stride : dst_tight;
        if (ss < src_tight || ds < dst_tight) return HVC_E_INVALID_ARG;
        if (ss >= (1ull << 32) || ds >= (1ull << 32)) return HVC_E_TOO_LARGE;
        const bool need_h = im.out_w != im.w, need_v = im.out_h != im.h || !need_h; // (neither: the copy, through the vertical pass)
        const bool both = need_h && need_v;
        // the intermediate of this image: out_w x h, rows on 4 bytes, the image (every plane) on 64
        const unsigned long long ms = (dst_tight + 3) & ~(unsigned long long)3;
        unsigned long long mid0 = 0;
        if (both) {
            mid0 = ((unsigned long long)plan.mid_bytes + 63) & ~(unsigned long long)63;
            plan.mid_bytes = (size_t)(mid0 + ms * (unsigned long long)im.h * planes);
        }
        unsigned rec_h = 0, rec_v = 0;
        int r;
        if (need_h && (r = plan_table(plan, im.w, im.out_w, filter, rec_h))) return r;
        if (need_v && (r = plan_table(plan, im.h, im.out_h, im.out_h == im.h ? (int)HVC_RESIZE_BOX : filter, rec_v))) return r;
        for (unsigned p = 0; p < planes; p++) {
            if (need_h) {
                ResizeImageK k;
                std::memset(&k, 0, sizeof k);
                k.src_base = (unsigned long long)im.src_offset + p * ss * (unsigned long long)im.h;
                k.src_stride = ss;
                k.dst_sel = both ? 1 : 0;
                k.dst_base = both ? mid0 + p * ms * (unsigned long long)im.h : (unsigned long long)im.dst_offset + p * ds * (unsigned long long)im.out_h;
                k.dst_stride = both ? ms : ds;
                k.rec0 = rec_h, k.tap_stride = (unsigned)im.out_w;
                k.n_out = (unsigned)im.out_w, k.rows = (unsigned)im.h, k.ch = ch;
                k.row_bytes = (unsigned)dst_tight;
                k.groups = (unsigned)im.out_w, k.magic = magic_of(k.groups);
                const unsigned long long lanes = (unsigned long long)im.out_w * (unsigned)im.h;
                // row = umulhi(t, magic) is exact for t * groups < 2^32
                if (lanes * k.groups >= (1ull << 32)) return HVC_E_TOO_LARGE;
                k.lanes = (unsigned)lanes;
                if ((r = add_units(plan.h, k, (lanes + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT, f))) return r;
            }
            if (need_v) {
                ResizeImageK k;
                std::memset(&k, 0, sizeof k);
                k.src_sel = both ? 1 : 0;
                k.src_base = both ? mid0 + p * ms * (unsigned long long)im.h : (unsigned long long)im.src_offset + p * ss * (unsigned long long)im.h;
                k.src_stride = both ? ms : ss;
                k.dst_base = (unsigned long long)im.dst_offset + p * ds * (unsigned long long)im.out_h;
                k.dst_stride = ds;
                k.rec0 = rec_v, k.tap_stride = (unsigned)im.out_h;
                k.n_out = (unsigned)im.out_h, k.rows = (unsigned)im.h, k.ch = ch;
                k.row_bytes = (unsigned)dst_tight;
                k.lanes = (k.row_bytes + 3) / 4;
                k.groups = (k.lanes + HVC_MIXED_UNIT - 1) / HVC_MIXED_UNIT, k.magic = magic_of(k.groups);
                const unsigned long long units = (unsigned long long)k.groups * (unsigned)im.out_h;
                if (units * k.groups >= (1ull << 32)) return HVC_E_TOO_LARGE; // (row = umulhi(u, magic), as above)
                const unsigned long long sa = both ? 0 : (unsigned long long)src_addr;
                k.vec = ((sa + k.src_base) | k.src_stride | ((unsigned long long)dst_addr + k.dst_base) | k.dst_stride) % 4 == 0;
                if ((r = add_units(plan.v, k, units, f))) return r;
            }
        }
    }
    return HVC_OK;
}

} // namespace

int resize_plan_build(const ResizeImage *images, const int *list, int n_list, int layout, int filter, uintptr_t src_addr,
                      uintptr_t dst_addr, ResizePlan &plan) {
    plan.clear();
    const int r = build(images, list, n_list, layout, filter, src_addr, dst_addr, plan);
    if (r) plan.clear();
    return r;
}

} // namespace hvc
