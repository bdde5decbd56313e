// hvc_mixed_encode_plan.h -- the host plan of a MIXED ENCODE batch (internal): frames of different geometry and quantiser
// tables in one launch of k_encode_mixed (hvc_mixed_encode.hip).  Plain C++, no HIP: hvc_mixed_encode_plan.cpp builds the
// tables the kernel reads from device memory, and the stand-alone program tests/host_harness/mixed_encode_plan_harness.cpp
// runs it under sanitizers.
//
//   plane descriptors, work map   mixed_plan_build's (hvc_mixed_plan.h): they do not depend on the direction
//   table entries                 the DISTINCT quantiser tables of the listed planes (deduplicated by content, in the order
//                                 mixed_plan_build meets them: a descriptor's `table` indexes both), each as the 64
//                                 reciprocals the forward quantiser multiplies by, zig-zag order
#ifndef HVC_MIXED_ENCODE_PLAN_H
#define HVC_MIXED_ENCODE_PLAN_H

#include "hvc_mixed_plan.h"

namespace hvc {

// What the forward quantiser multiplies a coefficient by in place of dividing by 4 t: fl((1 + 2^-16) / (4 t)).  One
// expression for k_encode (EncodeParams::qrcp) and k_encode_mixed (MixedEncTableK): tests/test_quant_division.py proves,
// exhaustively over t in 1..255 and |f| <= 2^15, that the product rounds to the model's quotient.
inline float encode_quant_reciprocal(unsigned t) { return (float)((1.0 + 1.0 / 65536.0) / (4.0 * (double)t)); }

struct MixedEncTableK { // 256 bytes
    float qrcp[64];     // encode_quant_reciprocal of the table's entries, zig-zag order
};

struct MixedEncodePlan {
    std::vector<MixedPlaneK> planes;
    std::vector<MixedEncTableK> tables;
    std::vector<int> qt;       // the entries themselves, 64 per table in zig-zag order (the libjpeg-exact block stage's multipliers
                               // are made from them: libjpeg_mixed_tables_build, hvc_libjpeg_encode_plan.h)
    std::vector<unsigned> map; // unit -> plane
    unsigned long long blocks = 0;
};

// Frame f of the set is infos[f].layout / .qtabs with its padded pixel record at pixel_offsets[f] (bytes) and its
// coefficient record at coef_offsets[f] (int16 elements); frames[0 .. n_list) names the frames to plan (nullptr: all).
// HVC_E_INVALID_ARG: a component with blocks_w or blocks_h of 0 (the model's encoder has no empty plane), and whatever
// mixed_plan_build answers with it; HVC_E_RANGE: an entry of a listed plane's table that is 0 or above 255 (the model's
// encoder tables are 8-bit); HVC_E_ALIGNMENT / HVC_E_TOO_LARGE: as mixed_plan_build.
int mixed_encode_plan_build(const hvc_jpeg_info *infos, const size_t *coef_offsets, const size_t *pixel_offsets, const int *frames,
                            int n_list, MixedEncodePlan &plan);

// hvc_jpeg_encoder_mixed_layout of include/hvc_jpeg.h
int encoder_mixed_layout(const int *widths, const int *heights, const int *chromas, const int *qualities, int n_frames, size_t align,
                         hvc_jpeg_info *infos, int *status, size_t *pixel_offsets, size_t *coef_offsets, size_t *pixel_total,
                         size_t *coef_total);

} // namespace hvc
#endif
