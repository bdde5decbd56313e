// hvc_mixed_libjpeg.h -- parameter block and launchers of the libjpeg-exact kernels over a mixed batch (internal):
// k_islow_mixed and k_ycc_to_rgb_fancy_mixed, hvc_mixed_libjpeg.hip (hvc_set_mixed_arithmetic HVC_ARITH_LIBJPEG).  The tables
// come from hvc_mixed_plan.h / hvc_mixed_rgb_plan.h, in device memory.
#ifndef HVC_MIXED_LIBJPEG_H
#define HVC_MIXED_LIBJPEG_H

#include <hip/hip_runtime.h>

#include "hvc_mixed_plan.h"
#include "hvc_mixed_rgb.h"

namespace hvc {

struct MixedIslowParams {
    const int16_t *coefs;
    uint8_t *pixels;
    const MixedPlaneK *planes;   // device
    const unsigned *pairs;       // device: HVC_ISLOW_PAIR_WORDS per table of the plan (mixed_islow_pairs_build), by MixedPlaneK::table
    const unsigned *map;         // device: n_units entries
    unsigned n_units;
    int all_wide;                // hvc_set_decode_kernel(ctx, 2): every block takes the int64 path (nothing is counted)
    unsigned long long *wide_total; // receives the number of blocks that took the int64 path (cleared by the caller)
    int xcd_map;                 // xcd_work with gridDim.y == 1 (hvc_kernels.h); 0: groups as dispatched
    unsigned xcd_magic;
};

// k_islow_mixed over all units; k0 / k1 (optional) bracket it
hipError_t launch_islow_mixed(const MixedIslowParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);
// k_ycc_to_rgb_fancy_mixed over all units of a plan of mixed_rgb_plan_build; k0 / k1 (optional) bracket it
hipError_t launch_ycc_to_rgb_fancy_mixed(const MixedRgbParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);

} // namespace hvc
#endif
