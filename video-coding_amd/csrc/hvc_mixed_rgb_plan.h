// hvc_mixed_rgb_plan.h -- the host plan of the colour pass over a MIXED batch (internal): images of different size and
// sampling in one launch of k_ycc_to_rgb_mixed (hvc_mixed_rgb.hip).  Plain C++, no HIP: hvc_mixed_rgb_plan.cpp builds the two
// tables the kernel reads from device memory, and the stand-alone program tests/host_harness/mixed_rgb_plan_harness.cpp runs
// it under sanitizers.  The way back, k_rgb_to_ycc_mixed, reads the same two tables: mixed_rgb_encode_plan_build below
// (tests/host_harness/mixed_rgb_encode_plan_harness.cpp).
//
//   image descriptors  one per listed frame with width * height > 0, in list order
//   work map           one image index per work unit; a unit = 64 consecutive LANES of ONE image = one wavefront, so that
//                      everything a wavefront looks up is wave-uniform; a workgroup takes HVC_MIXED_GROUP consecutive units
// A lane is what a lane of k_ycc_to_rgb is: 8 columns of one image row (4:2:0: of two rows); an image has
// ceil(w / 8) lanes per lane row and h (4:2:0: ceil(h / 2)) lane rows, lane t of the image = lane row t / groups, column
// group t % groups, the division by the descriptor's magic reciprocal.
#ifndef HVC_MIXED_RGB_PLAN_H
#define HVC_MIXED_RGB_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "hvc_mixed_plan.h" /* HVC_MIXED_UNIT, HVC_MIXED_GROUP, HVC_MIXED_MAX_UNITS */

// by the scan's sampling factors: HVC_YUV_420 / 422 / 444 / 400, 0 = none of them (the rule of hvc_jpeg_decode_rgb)
int rgb_sampling_of(const hvc_jpeg_info &info);
// the chroma samples the RGB image reads: ceil(width / 2) x ceil(height / 2) for 4:2:0, ...
void rgb_chroma_window(int sampling, int width, int height, int &cw, int &ch);

namespace hvc {

struct MixedRgbImageK {             // 120 bytes
    unsigned long long y_base, cb_base, cr_base; // bytes from the launch's plane pointer (grey: cb = cr = 0)
    unsigned long long rgb_base;                 // bytes from the launch's RGB pointer
    unsigned long long y_stride, cb_stride, cr_stride; // bytes per row of each plane
    unsigned long long row_stride, plane_stride; // of the RGB image (plane_stride = row_stride * h: the planar layout)
    int w, h, cw, ch;                // image size; valid chroma samples (where the neighbours clamp)
    int sampling;                    // HVC_YUV_420 / 422 / 444 / 400
    int vec_y, vec_c, vec_rgb;       // ACTUAL addresses and strides allow the 8 / 4-byte forms (RgbOp's flags, per image)
    unsigned groups, magic;          // lanes per lane row = ceil(w / 8); ceil(2^32 / groups), 0 for groups == 1
    unsigned lanes;                  // groups * lane rows
    unsigned unit0;                  // its first work unit
};

struct MixedRgbPlan {
    std::vector<MixedRgbImageK> images;
    std::vector<unsigned> map;     // unit -> image
    std::vector<int> frame;        // image -> the frame (index into infos) it is
    unsigned long long lanes = 0;
};

// bytes per tight row, rows from the first to the last (planar: the three planes follow one another: 3 h)
inline size_t mixed_rgb_row_bytes(int layout, int width) { return layout == HVC_RGB_PLANAR ? (size_t)width : (size_t)3 * width; }
inline size_t mixed_rgb_rows(int layout, int height) { return layout == HVC_RGB_PLANAR ? (size_t)3 * height : (size_t)height; }
// from the first byte of an image to the last one written (0: an empty image)
inline size_t mixed_rgb_span(int layout, int width, int height, size_t row_stride) {
    return width < 1 || height < 1 ? 0 : (mixed_rgb_rows(layout, height) - 1) * row_stride + mixed_rgb_row_bytes(layout, width);
}

// The descriptor builder.  Frame f of the set: infos[f].width x .height, its sampling by rgb_sampling_of, its planes at
// yuv_offsets[f] + infos[f].layout[k].plane_offset with .stride, its chroma window by rgb_chroma_window, its RGB image at
// rgb_offsets[f] with rows rgb_row_strides[f] apart (rgb_row_strides == nullptr: tight rows).  frames[0 .. n_list) names
// the frames to plan, in launch order (nullptr: 0 .. n_list - 1) -- a list, not a range.  yuv_addr / rgb_addr: the
// addresses the offsets count from (only their low bits matter: the vec_* flags follow the actual addresses).  decoded: the
// planes are what the block stage writes for infos[f].layout, so every component read must name its blocks.
// HVC_E_INVALID_ARG: a negative size, a sampling that is none of the four, a stride below its row, a window outside its
// decoded plane (components that name their blocks; decoded: all must), a bad layout; HVC_E_TOO_LARGE: an image beyond the lane arithmetic
// (a side above 2^24, lanes * groups >= 2^32) or more than HVC_MIXED_MAX_UNITS units.
int mixed_rgb_plan_build(const hvc_jpeg_info *infos, const size_t *yuv_offsets, const size_t *rgb_offsets, const size_t *rgb_row_strides,
                         int layout, const int *frames, int n_list, uintptr_t yuv_addr, uintptr_t rgb_addr, bool decoded,
                         MixedRgbPlan &plan, int n = 8);
// (n = 4, 2, 1: infos[] are SCALED infos, their planes what the scaled block stage writes: a window must lie inside
// n * blocks_w x n * blocks_h)

// The same tables for the ENCODE direction, k_rgb_to_ycc_mixed: frame f's RGB image at rgb_offsets[f] is read, its planes at
// yuv_offsets[f] + infos[f].layout[k].plane_offset are written.  A lane is what a lane of k_rgb_to_ycc is: ceil(w / 8) lanes
// per lane row, h lane rows (4:2:0: h / 2 -- sizes are even here, not rounded up), chroma rows of w / 2 samples (4:4:4: w);
// cw / ch of the descriptor hold that chroma size.  Arguments as mixed_rgb_plan_build.  HVC_E_INVALID_ARG for the whole
// plan: an odd width under 4:2:0 / 4:2:2, an odd height under 4:2:0 (Yuv.assert_is_420 / _422), a sampling that is not one of
// those three (grey among them), a stride below its row, samples outside a component that names its blocks, a negative size,
// a bad layout; HVC_E_TOO_LARGE as there.  A frame without a pixel gets no descriptor.
int mixed_rgb_encode_plan_build(const hvc_jpeg_info *infos, const size_t *yuv_offsets, const size_t *rgb_offsets,
                                const size_t *rgb_row_strides, int layout, const int *frames, int n_list, uintptr_t yuv_addr,
                                uintptr_t rgb_addr, MixedRgbPlan &plan);

// hvc_jpeg_encoder_mixed_rgb_layout of include/hvc_jpeg.h
int encoder_mixed_rgb_layout(const int *widths, const int *heights, const int *chromas, const int *qualities, int n_frames, int layout,
                             size_t align, size_t row_align, hvc_jpeg_info *infos, int *status, size_t *rgb_offsets,
                             size_t *rgb_row_strides, size_t *rgb_total, size_t *pixel_offsets, size_t *coef_offsets, size_t *pixel_total,
                             size_t *coef_total);

// hvc_jpeg_mixed_rgb_layout of include/hvc_jpeg.h
int mixed_rgb_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int layout, size_t align, size_t row_align,
                     hvc_jpeg_info *infos, int *status, size_t *rgb_offsets, size_t *rgb_row_strides, size_t *total_bytes);
// hvc_jpeg_mixed_scaled_rgb_layout of include/hvc_jpeg.h
int mixed_scaled_rgb_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int scale_denom, int layout, size_t align,
                            size_t row_align, hvc_jpeg_info *infos, hvc_jpeg_info *scaled, int *status, size_t *rgb_offsets,
                            size_t *rgb_row_strides, size_t *total_bytes);

} // namespace hvc
#endif
