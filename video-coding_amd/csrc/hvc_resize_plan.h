// hvc_resize_plan.h -- the host plan of the resampling step over a MIXED set (internal): RGB images of different size, each to
// a size of its own, in one launch per pass of k_resize_h_mixed / k_resize_v_mixed (hvc_resize.hip).  Plain C++, no HIP:
// hvc_resize_plan.cpp builds the tables the kernels read from device memory, and the stand-alone program
// tests/host_harness/resize_plan_harness.cpp runs it under sanitizers.  The definition: include/hvc_jpeg.h, Resizing
// (tools/resize_reference.py in numpy).  hvc_resize_plan.cpp is compiled with -ffp-contract=off: a fused multiply-add changes
// the last bit of a weight and with it a tap.
//
//   axis tables        one per distinct (n_in, n_out, filter) of the set -- under resize_plan_build_opts (n_in, n_out, filter, bits
//                      of in0, bits of in1, mirrored, shift), at the end of this file: per output position a record (xmin, count, first
//                      tap) and the 22-bit taps, stored TRANSPOSED -- tap i of position p is taps[first + i * n_out], first =
//                      the table's base + p -- so that consecutive lanes (consecutive positions) read consecutive words
//   image descriptors  per pass, one per image (planar: one per plane -- three one-channel images, so that no pass reads
//                      across a plane boundary)
//   work map           per pass, one descriptor index per work unit; a unit = one wavefront of ONE image
// The passes (the order is part of the definition): horizontal first, source -> an 8-bit intermediate of out_w x h, then
// vertical, intermediate -> destination.  An axis with n_out == n_in (and, under a box, the whole axis as its window) is skipped: the image gets no descriptor in that pass
// and the other pass goes straight from the source to the destination.  An image whose two axes are both skipped is a copy:
// it goes through the vertical pass with the identity table (h -> h under box: one tap of 2^22 per row).
//   horizontal lanes   one lane per output sample position of one source row, all its channels: out_w lanes per row, h rows,
//                      lane t = row t / out_w, position t % out_w (the descriptor's magic reciprocal); a unit = 64
//                      consecutive lanes of the image
//   vertical lanes     one lane per 4 consecutive BYTES of one output row (the pass does not know channels); a unit = 64
//                      consecutive lanes of ONE ROW, so that the row's record and taps are wave-uniform: ceil(lanes per
//                      row / 64) units per row, out_h rows, unit u = row u / units per row (magic), segment u % units per row
#ifndef HVC_RESIZE_PLAN_H
#define HVC_RESIZE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "hvc_mixed_plan.h" /* HVC_MIXED_UNIT, HVC_MIXED_GROUP, HVC_MIXED_MAX_UNITS */

// The documented bounds (include/hvc_jpeg.h): taps per output position of one axis, and 32-bit words of all tables of one call.
// 8192 -> 1 under bicubic would be 8192 taps per sample: such an image is refused with HVC_E_TOO_LARGE.
// (HVC_RESIZE_MAX_TAPS = 2048: the public header's)
#define HVC_RESIZE_MAX_TABLE_WORDS (1u << 24)
#define HVC_RESIZE_PRECISION_BITS 22

namespace hvc {

struct ResizeRecK {   // 12 bytes: one output position of one axis
    unsigned xmin;    // first input sample it reads
    unsigned count;   // taps
    unsigned first;   // index of tap 0 in the launch's tap array; tap i at first + i * the descriptor's tap_stride
};

struct ResizeImageK {               // 96 bytes: one image (one plane) of one pass
    unsigned long long src_base, dst_base;     // bytes from the pass's source / destination pointer (src_sel / dst_sel)
    unsigned long long src_stride, dst_stride; // bytes per row
    unsigned rec0;                  // its table: the record of output position 0
    unsigned tap_stride;            // words between consecutive taps of one position = n_out of the table
    unsigned n_out;                 // horizontal: output samples per row; vertical: output rows
    unsigned rows;                  // horizontal: rows (= h of the source; both axes under a box: the rows of the vertical
                                    // pass's window); vertical: the source rows from src_base on
    unsigned ch;                    // horizontal: channels per sample (3 interleaved, 1 planar)
    unsigned row_bytes;             // vertical: bytes per output row
    unsigned groups, magic;         // horizontal: lanes per row and ceil(2^32 / groups); vertical: units per row and its
                                    // reciprocal (0 for groups == 1)
    unsigned lanes;                 // horizontal: n_out * rows; vertical: lanes per ROW = ceil(row_bytes / 4)
    unsigned units, unit0;          // its work units, the first of them
    unsigned src_sel, dst_sel;      // 0: the call's source / destination, 1: the intermediate
    unsigned vec;                   // vertical: source and destination rows all start on 4 bytes: dword loads and stores
                                    // (typed output: the SOURCE rows alone)
    unsigned dvec;                  // vertical, typed output: destination rows all start on 4 * out_elem bytes: one 8- / 16-byte store
    unsigned chan;                  // vertical, typed output: the plane's channel (planar); interleaved: 3, the channel of a
                                    // sample is its index in the row modulo 3
};

struct ResizePass {
    std::vector<ResizeImageK> images;
    std::vector<unsigned> map;      // unit -> descriptor
    std::vector<int> image;         // descriptor -> index into the caller's image list entries (the image it belongs to)
};

struct ResizeImage {                // one image as the caller describes it
    int w = 0, h = 0, out_w = 0, out_h = 0;
    size_t src_offset = 0, src_row_stride = 0; // a stride of 0: tight rows
    size_t dst_offset = 0, dst_row_stride = 0;
};

struct ResizeTableKey {
    int n_in, n_out, filter;
    unsigned rec0;
    // the box forms: the window as the bits of two IEEE singles (the whole axis: 0 and n_in), the records in reverse output
    // order (mirror), and what was subtracted from every xmin (a vertical table: its own xmin[0]; horizontal: 0)
    uint32_t in0_bits = 0, in1_bits = 0;
    int mirrored = 0;
    unsigned shift = 0;
};

struct ResizePlan {
    ResizePass h, v;
    std::vector<ResizeRecK> recs;
    std::vector<int> taps;
    std::vector<ResizeTableKey> tables; // the distinct tables, in the order they were first needed
    size_t mid_bytes = 0;               // the intermediate: every image's out_w x (the rows of its window) rows, row starts on 4
                                        // bytes, images on 64
    int out_elem = 0;                   // bytes per output element: 0 (8-bit samples: k_resize_v_mixed) or 2 / 4 (k_resize_v_mixed_lut)
    void clear() { *this = ResizePlan(); }
};

// One axis, the definition itself: recs[p] = (xmin, count, first = p) and taps transposed with stride n_out (kmax * n_out
// words, zeros behind a position's count).  HVC_E_INVALID_ARG: a size below 1, an unknown filter; HVC_E_TOO_LARGE: a size
// above 2^24, more than HVC_RESIZE_MAX_TAPS taps at a position, a table above HVC_RESIZE_MAX_TABLE_WORDS, or a position that
// fails 255 * SUM |k| + 2^21 < 2^31 or |k| < 2^23 (the kernels' int32 accumulator and 24-bit multiply).
int resize_axis_build(int n_in, int n_out, int filter, std::vector<ResizeRecK> &recs, std::vector<int> &taps);
// the same verdict without the tables (what the file pipeline gives a file as its status): both axes of one image
int resize_image_status(int w, int h, int out_w, int out_h, int filter);

inline size_t resize_row_bytes(int layout, int width) { return layout == HVC_RGB_PLANAR ? (size_t)width : (size_t)3 * width; }
inline size_t resize_rows(int layout, int height) { return layout == HVC_RGB_PLANAR ? (size_t)3 * height : (size_t)height; }
// from the first byte of an image to the last one read or written
inline size_t resize_span(int layout, int width, int height, size_t row_stride) {
    return (resize_rows(layout, height) - 1) * row_stride + resize_row_bytes(layout, width);
}

// The plan of a set: images[list[0 .. n_list)] (list == nullptr: 0 .. n_list - 1), one layout and one filter per call.
// src_addr / dst_addr: the addresses the offsets count from (only their low bits matter: the vertical pass's `vec` follows
// the actual addresses); the intermediate is taken to start on 64 bytes.  Planar planes lie row_stride * height apart.
// HVC_E_INVALID_ARG: a size below 1, a stride below the row, an unknown filter or layout; HVC_E_TOO_LARGE: what
// resize_axis_build refuses, lanes beyond the magic division (lanes * lanes per row >= 2^32), more than HVC_MIXED_MAX_UNITS
// units in a pass, all tables together above HVC_RESIZE_MAX_TABLE_WORDS.  A refused set leaves an empty plan.
int resize_plan_build(const ResizeImage *images, const int *list, int n_list, int layout, int filter, uintptr_t src_addr,
                      uintptr_t dst_addr, ResizePlan &plan);

// ---- the box, the mirror and the typed output (include/hvc_jpeg.h: Box, Mirror, Typed output) ----
// One axis under a window [in0, in1) of IEEE singles: scale = (double)(float)(in1 - in0) / n_out, center = (double)in0 + (xx +
// 0.5) * scale, the rest as resize_axis_build -- which is this with (0, n_in, false, 0).  reversed: the record and taps of output
// position p are those of position n_out - 1 - p (the mirror: no kernel knows about it).  shift: subtracted from every xmin
// (at most the smallest of them).  HVC_E_INVALID_ARG on top of resize_axis_build's: a non-finite value, in0 < 0, in1 > n_in,
// (float)(in1 - in0) <= 0 (Pillow lets a zero span through; this does not).
int resize_axis_build_box(int n_in, int n_out, int filter, float in0, float in1, bool reversed, unsigned shift,
                          std::vector<ResizeRecK> &recs, std::vector<int> &taps);
// [first, last) of the samples the axis reads: xmin[0] and xmin[n_out - 1] + count[n_out - 1]; the axis must be one that
// resize_axis_build_box accepts
void resize_axis_window(int n_in, int n_out, int filter, float in0, float in1, unsigned &first, unsigned &last);
// an axis is skipped iff n_out == n_in and the window is the whole axis
inline bool resize_axis_skipped(int n_in, int n_out, float in0, float in1) { return n_out == n_in && in0 == 0.0f && in1 == (float)n_in; }
// resize_image_status under a box (x0, y0, x1, y1; nullptr: the whole image) and a mirror flag
int resize_image_status_box(int w, int h, int out_w, int out_h, int filter, const float *box, int mirror);

// What a call may ask on top of resize_plan_build; indexed like `images` (by image, not by list position).
struct ResizePlanOpts {
    const float *boxes = nullptr;    // nullptr, or 4 per image: x0, y0, x1, y1 in the image's coordinates
    const uint8_t *mirror = nullptr; // nullptr, or 1 per image: != 0 reverses every output row
    int out_elem = 0;                // 0: 8-bit samples; 2 / 4: bytes per output element (the destination's strides, offsets and
                                     // row lengths are bytes: a tight row is resize_row_bytes * out_elem)
};
// resize_plan_build with them (all-default opts: the very same plan).  The differences:
//   tables       keyed (n_in, n_out, filter, bits of in0, bits of in1, mirrored, shift): with a box of its own an image has
//                tables of its own, so a large set meets HVC_RESIZE_MAX_TABLE_WORDS (HVC_E_TOO_LARGE) sooner
//   row window   when both axes run the horizontal pass covers only source rows [ymin[0], ymin[H - 1] + count[H - 1]): its
//                descriptor starts at that row and has that many rows, and the intermediate (mid_bytes) holds only them
//   vertical     every vertical table is shifted by its ymin[0] and the descriptor's src_base starts at that row (without a
//                box ymin[0] is 0: nothing changes)
//   mirror       the horizontal axis runs even where it would be skipped (the identity table, box n -> n), records reversed
//   typed        out_elem 2 / 4: every image ends in the vertical pass (the identity table where that axis is skipped, as
//                the copy does), whose descriptors carry dvec and chan; dst strides are checked against the typed row
// HVC_E_INVALID_ARG: an out_elem other than 0, 2, 4; a box resize_axis_build_box refuses.
int resize_plan_build_opts(const ResizeImage *images, const int *list, int n_list, int layout, int filter, uintptr_t src_addr,
                           uintptr_t dst_addr, const ResizePlanOpts &opts, ResizePlan &plan);

} // namespace hvc
#endif
