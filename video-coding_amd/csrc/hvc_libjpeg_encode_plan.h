// hvc_libjpeg_encode_plan.h -- the host arithmetic of the libjpeg-exact encoder (hvc_set_encode_libjpeg; include/hvc_jpeg.h
// "Encoding bit-exact to libjpeg"): the quantiser's division magics and the dummy blocks' source index.  Plain C++ (no HIP),
// usable without a GPU: tests/host_harness/libjpeg_encode_plan_harness.cpp exhausts both under the sanitizers.
#ifndef HVC_LIBJPEG_ENCODE_PLAN_H
#define HVC_LIBJPEG_ENCODE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/hvc_jpeg.h"
#include "hvc_fdct_islow_spec.h"
#include "hvc_mixed_rgb_plan.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HVC_LJE_HD __host__ __device__ __forceinline__
#else
#define HVC_LJE_HD inline
#endif

namespace hvc {

// The quantiser divides n = |t| + 4 q by d = 8 q.  One multiplier per table entry: m = ceil(2^26 / d), and
// n / d == (n * m) >> 26 for every n <= HVC_FI_T_MAX + 4 q: m d = 2^26 + e with 0 <= e < d, so n m / 2^26 = n / d + n e / (d 2^26),
// and the second term is below 1 / d while n e < 2^26 -- n <= 8192 + 1020, e < 2040, n e < 1.9e7 < 2^26.  26 bits because both
// factors then fit the 24 bits of a full-rate multiply: d >= 8 gives m <= 2^23, and the kernel forms (n << 6) * m, n << 6 < 2^20,
// whose high dword (v_mul_hi_u32_u24) is (n * m) >> 26.
#define HVC_LJE_MAGIC_BITS 26
#define HVC_LJE_NUMERATOR_SHIFT (32 - HVC_LJE_MAGIC_BITS)
uint32_t libjpeg_quant_magic(int q);
// what the kernel computes with it (the harness compares this with C's /)
HVC_LJE_HD uint32_t libjpeg_quant_divide(uint32_t n, uint32_t m) { return (uint32_t)(((uint64_t)n * m) >> HVC_LJE_MAGIC_BITS); }
HVC_LJE_HD int libjpeg_quantise(int t, uint32_t m, uint32_t half) {
    const uint32_t a = (uint32_t)(t < 0 ? -t : t);
    const int q = (int)libjpeg_quant_divide(a + half, m);
    return t < 0 ? -q : q;
}
// zig-zag tables with entries in 1 .. 255 -> per table and NATURAL position k the magic and the rounding term 4 q of
// table[zig-zag position of k] (the kernel walks its results in natural order)
void libjpeg_encode_tables(const uint16_t *qtabs, int n_qtabs, uint32_t *magic, uint32_t *half);

// A component plane of bw x bh blocks whose first real_w x real_h are real (1 <= real_w <= bw, bw - real_w < h; the same
// downward with v), sampling factors h x v.  The block whose DC block (bx, by) takes, as bx + by * bw: itself when real.
// The definition walks libjpeg's MCU buffer (jccoefct.c compress_data): a dummy in a real row copies the block on its left;
// every block of a dummy row copies the LAST block of the row above inside its MCU; both chain through dummies.
int libjpeg_dummy_source_walk(int bx, int by, int bw, int real_w, int real_h, int h);
// The same in closed form (what k_dummy_blocks evaluates; the harness holds it to the walk): the chain of a dummy row ends in
// the last real row at the MCU's last column, or at the last real column where that one is a dummy too.
HVC_LJE_HD int libjpeg_dummy_source(int bx, int by, int bw, int real_w, int real_h, int h) {
    if (by >= real_h) {
        const int last = bx / h * h + h - 1;
        return (last < real_w ? last : real_w - 1) + (real_h - 1) * bw;
    }
    return (bx < real_w ? bx : real_w - 1) + by * bw;
}
// The i-th dummy block of the plane, i < libjpeg_dummy_count: first the dummies of the real rows, row by row, then the dummy
// rows whole.
HVC_LJE_HD int libjpeg_dummy_count(int bw, int bh, int real_w, int real_h) { return bw * bh - real_w * real_h; }
HVC_LJE_HD void libjpeg_dummy_at(int i, int bw, int real_w, int real_h, int &bx, int &by) {
    const int right = (bw - real_w) * real_h;
    if (i < right) {
        by = i / (bw - real_w);
        bx = real_w + i - by * (bw - real_w);
    } else {
        i -= right;
        by = real_h + i / bw;
        bx = i - (by - real_h) * bw;
    }
}

// The mixed block stage (k_fdct_islow_mixed): one record per distinct table of a MixedEncodePlan, beside the plan image
struct FdctIslowTableK { // 512 bytes
    uint32_t magic[64];  // libjpeg_encode_tables' words of the table, natural order
    uint32_t half[64];
};
// qt: 64 entries per table in zig-zag order, each in 1 .. 255 (MixedEncodePlan::qt)
void libjpeg_mixed_tables_build(const std::vector<int> &qt, std::vector<FdctIslowTableK> &tables);
// ... and its dummy pass (k_dummy_blocks_mixed): per dummy block of the listed frames where its record and its source block's
// start, in int16 elements from the launch's coefficient pointer.  Frame f's record is at coef_offsets[f]; frames[0 .. n_list)
// names the frames (nullptr: 0 .. n_list - 1), as for mixed_encode_plan_build.  A component whose info states no size
// (actual_width or actual_height <= 0: a hand-made info) has no dummy block.  HVC_E_INVALID_ARG: a component whose
// ceil(actual / 8) is not inside its plane.
struct DummyPairK {
    unsigned long long dst, src;
};
int libjpeg_mixed_dummies_build(const hvc_jpeg_info *infos, const size_t *coef_offsets, const int *frames, int n_list,
                                std::vector<DummyPairK> &pairs);

// The colour pass RGB -> planes (k_rgb_to_ycc_libjpeg[_mixed], hvc_rgb_libjpeg_dev.h) runs on a plan of
// mixed_rgb_encode_plan_build (hvc_mixed_rgb_plan.h: its checks, bases and strides) with the lane grid of the OUTPUT planes: a lane
// is 8 luma columns of one row (4:2:0: two rows); pad = every component is written up to ceil(actual / 8) * 8 both ways, so the
// grid covers the wider of the luma extent and the chroma extent at full size.  Rewrites groups / magic / lanes / unit0 of every
// image and the map (a unit is 64 lanes of one image).  infos (pad only; plan.frame indexes it): HVC_E_INVALID_ARG where a
// padded component does not fit the plane its info lays out (8 * blocks, and the stride).
int libjpeg_rgb_plan_lanes(MixedRgbPlan &plan, bool pad, const hvc_jpeg_info *infos);
// the lane grid of one image (what libjpeg_rgb_plan_lanes applies)
void libjpeg_rgb_lane_grid(int w, int h, int sampling, bool pad, unsigned &lanes_x, unsigned &lanes_y);

// pad_frame's sibling under the setting (hvc_mixed_encode_chunks.h): the tight planes of a frame (component i is
// comp[i].actual_width x actual_height, back to back) into the padded pixel record of info.layout, the last column repeated to
// the right and the last row downward (where pad_frame leaves zeros).  The dummy blocks' samples are never looked at.
void pad_frame_replicate(const hvc_jpeg_info &info, const uint8_t *src, uint8_t *rec);
// one plane: sw x sh samples at src (stride sw) -> pw x ph at dst (stride `stride`); sw, sh >= 1
void pad_plane_replicate(const uint8_t *src, int sw, int sh, uint8_t *dst, int pw, int ph, size_t stride);

} // namespace hvc
#endif
