// hvc_resize.h -- parameter block and launchers of the resampling passes over a mixed set (internal): k_resize_h_mixed and
// k_resize_v_mixed (and its typed form k_resize_v_mixed_lut), hvc_resize.hip.  The tables come from hvc_resize_plan.h, in device memory.
#ifndef HVC_RESIZE_H
#define HVC_RESIZE_H

#include <hip/hip_runtime.h>

#include "hvc_resize_plan.h"

namespace hvc {

struct ResizeParams {
    const uint8_t *src[2];          // [0] the call's source, [1] the intermediate (a descriptor's src_sel)
    uint8_t *dst[2];                // [0] the call's destination, [1] the intermediate (dst_sel)
    const ResizeImageK *images;     // device: the pass's descriptors
    const unsigned *map;            // device: n_units entries
    const ResizeRecK *recs;         // device: the records of all tables
    const int *taps;                // device: the taps of all tables
    unsigned n_units;
};

// one launch over all units of the pass; n_units == 0 (no image needs the pass) launches nothing
hipError_t launch_resize_h_mixed(const ResizeParams &P, hipStream_t s);
hipError_t launch_resize_v_mixed(const ResizeParams &P, hipStream_t s);
// the vertical pass of a plan made with out_elem = elem (2 or 4): k_resize_v_mixed_lut<elem>; lut: device memory, 3 * 256
// elements of elem bytes, [channel][sample], on elem bytes
hipError_t launch_resize_v_mixed_lut(const ResizeParams &P, const void *lut, int elem, hipStream_t s);

} // namespace hvc
#endif
