// hvc_mixed.h -- parameter block and launchers of the mixed block stage (internal): k_decode_mixed / k_decode_mixed_wide,
// hvc_mixed.hip, and k_decode_mixed_scaled, hvc_mixed_scaled.hip.  The tables come from hvc_mixed_plan.h, in device memory.
#ifndef HVC_MIXED_H
#define HVC_MIXED_H

#include <hip/hip_runtime.h>

#include "hvc_mixed_plan.h"

namespace hvc {

struct MixedParams {
    const int16_t *coefs;
    uint8_t *pixels;
    const MixedPlaneK *planes;   // device
    const MixedTableK *tables;   // device
    const unsigned *map;         // device: n_units entries
    unsigned n_units;
    int all_wide;                // hvc_set_decode_kernel(ctx, 2): every block goes to the list, i.e. through the int64 arithmetic
    // the fix-up list of the context (hvc_ctx.h fix_assign): ids unit * 64 + lane
    unsigned *fix_count, *fix_count_next, *fix_list;
    unsigned long long *wide_total;
    int wide_first;
    int xcd_map;                 // xcd_work with gridDim.y == 1 (hvc_kernels.h); 0: groups as dispatched
    unsigned xcd_magic;
};

// k_decode_mixed over all units, then k_decode_mixed_wide over the list; k0 / k1 (optional) bracket the first
hipError_t launch_decode_mixed(const MixedParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);

// k_decode_mixed_scaled<n> (hvc_mixed_scaled.hip), n = 4, 2, 1, over all units of a plan built for n: of the fix-up fields
// it takes wide_total alone (cleared by the caller; the blocks of the int64 branch are added to it)
hipError_t launch_decode_mixed_scaled(const MixedParams &P, int n, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);

} // namespace hvc
#endif
