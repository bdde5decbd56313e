// hvc_mixed_encode.h -- parameter block and launcher of the mixed FORWARD block stage (internal): k_encode_mixed,
// hvc_mixed_encode.hip.  The tables come from hvc_mixed_encode_plan.h, in device memory.
#ifndef HVC_MIXED_ENCODE_H
#define HVC_MIXED_ENCODE_H

#include <hip/hip_runtime.h>

#include "hvc_mixed_encode_plan.h"

namespace hvc {

struct MixedEncodeParams {
    const uint8_t *pixels;
    int16_t *coefs;
    const MixedPlaneK *planes;    // device
    const MixedEncTableK *tables; // device
    const unsigned *map;          // device: n_units entries
    unsigned n_units;
    int xcd_map;                  // xcd_work with gridDim.y == 1 (hvc_kernels.h); 0: groups as dispatched
    unsigned xcd_magic;
};

// k_encode_mixed over all units; k0 / k1 (optional) bracket it
hipError_t launch_encode_mixed(const MixedEncodeParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);

} // namespace hvc
#endif
