// hvc_mixed_plan.h -- the host plan of a MIXED batch (internal): frames of different geometry and quantiser tables in one
// launch of k_decode_mixed (hvc_mixed.hip).  Plain C++, no HIP: hvc_mixed_plan.cpp builds the three tables the kernels read
// from device memory, and the stand-alone program tests/host_harness/mixed_plan_harness.cpp runs it under sanitizers.
//
//   plane descriptors  one per non-empty component plane of the listed frames, in list order
//   table entries      the DISTINCT quantiser tables of those planes (deduplicated by content)
//   work map           one plane index per work unit; a unit = 64 consecutive blocks of ONE plane = one wavefront, so that
//                      everything a wavefront looks up is wave-uniform; a workgroup takes four consecutive units
// Which lookup was built (the map, not a search over unit prefix sums) and why: profiles/mixed_rocprofv3.txt.
#ifndef HVC_MIXED_PLAN_H
#define HVC_MIXED_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/hvc_jpeg.h"

#define HVC_MIXED_UNIT 64      /* blocks per work unit = lanes per wavefront */
#define HVC_MIXED_GROUP 4      /* units per workgroup */
#define HVC_MIXED_MAX_UNITS (1u << 26) /* a fix-list id is unit * 64 + lane in 32 bits */

namespace hvc {

struct MixedPlaneK {            // 48 bytes
    unsigned long long coef_base; // int16 elements from the launch's coefficient pointer
    unsigned long long pix_base;  // bytes from the launch's pixel pointer
    unsigned long long stride;    // bytes per pixel row
    int bw, nblk;                 // blocks per block row, blocks in the plane
    unsigned magic;               // ceil(2^32 / bw), 0 for bw == 1 (CompK::magic)
    int table;                    // index of its table entry
    unsigned unit0;               // its first work unit
    unsigned pad;
};

struct MixedTableK {            // 400 bytes
    unsigned qpair[32];           // per row r the operand pairs A, B, C, Z of hvc_idct_spec.h as lo | hi << 16 (DecodeParams::qpair)
    int qt[64];                   // the entries as ints, zig-zag order: the int64 kernel's form
    int ethr_packed;              // largest coefficient energy the int32 form accepts: (HVC_GUARD_D_PACKED / qmax)^2
    int wide;                     // an entry above 255: every block of its planes goes through the int64 kernel
    int pad[2];
};

struct MixedPlan {
    std::vector<MixedPlaneK> planes;
    std::vector<MixedTableK> tables;
    std::vector<unsigned> map;    // unit -> plane
    unsigned long long blocks = 0;
};

// The descriptor builder.  Frame f of the set is infos[f].layout / .qtabs with its coefficient record at coef_offsets[f]
// (int16 elements) and its pixel record at pixel_offsets[f] (bytes).  frames[0 .. n_list) names the frames to plan, in
// launch order (nullptr: 0 .. n_list - 1) -- a list, not a range: a batch pipeline leaves out the files whose scan failed.
// A component with blocks_w or blocks_h of 0 gets no descriptor; a set without a block gives an empty plan.
// HVC_E_ALIGNMENT: a coefficient plane not on 16 bytes, a pixel plane or stride not on 8; HVC_E_INVALID_ARG: a negative
// size, a table index outside the frame's tables, a stride below the row; HVC_E_TOO_LARGE: a plane beyond CompK's index
// range or more than HVC_MIXED_MAX_UNITS units.
int mixed_plan_build(const hvc_jpeg_info *infos, const size_t *coef_offsets, const size_t *pixel_offsets, const int *frames,
                     int n_list, MixedPlan &plan);

// hvc_jpeg_mixed_layout of include/hvc_jpeg.h
int mixed_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, size_t align, hvc_jpeg_info *infos, int *status,
                 size_t *pixel_offsets, size_t *total_bytes);

} // namespace hvc
#endif
