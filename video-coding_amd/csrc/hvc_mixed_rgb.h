// hvc_mixed_rgb.h -- parameter block and launcher of the colour pass over a mixed batch (internal): k_ycc_to_rgb_mixed and
// k_rgb_to_ycc_mixed, hvc_mixed_rgb.hip.  The tables come from hvc_mixed_rgb_plan.h, in device memory.
#ifndef HVC_MIXED_RGB_H
#define HVC_MIXED_RGB_H

#include <hip/hip_runtime.h>

#include "hvc_mixed_rgb_plan.h"

namespace hvc {

struct MixedRgbParams {
    const uint8_t *yuv;             // the planes: descriptor bases count from here
    uint8_t *rgb;                   // the images: rgb_base counts from here
    const MixedRgbImageK *images;   // device
    const unsigned *map;            // device: n_units entries
    unsigned n_units;
    int planar;                     // HVC_RGB_PLANAR (one call has one layout: a template parameter of the kernel)
};

// one launch over all units; k0 / k1 (optional) bracket it
hipError_t launch_ycc_to_rgb_mixed(const MixedRgbParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);
// the way back (k_rgb_to_ycc_mixed, tables from mixed_rgb_encode_plan_build): P.rgb is read, the planes at P.yuv are written
hipError_t launch_rgb_to_ycc_mixed(const MixedRgbParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);

} // namespace hvc
#endif
