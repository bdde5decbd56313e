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

// N = 8 / scale_denom, 0 for anything but 1, 2, 4, 8
inline int scaled_side(int scale_denom) {
    return scale_denom == 1 || scale_denom == 2 || scale_denom == 4 || scale_denom == 8 ? 8 / scale_denom : 0;
}
// hvc_jpeg_scaled_info's arithmetic; n = scaled_side(scale_denom) != 0
inline void scaled_info(const hvc_jpeg_info &in, int n, hvc_jpeg_info &out) {
    const hvc_jpeg_info src = in; // (in and out may be one object)
    auto up = [n](int x) { return (int)(((long long)x * n + 7) / 8); };
    out = src;
    out.width = up(src.width);
    out.height = up(src.height);
    size_t at = 0;
    for (int i = 0; i < src.n_comp && i < 4; i++) {
        hvc_jpeg_component &k = out.comp[i];
        k.actual_width = up(src.comp[i].actual_width);
        k.actual_height = up(src.comp[i].actual_height);
        k.decoded_width = src.comp[i].decoded_width / 8 * n;
        k.decoded_height = src.comp[i].decoded_height / 8 * n;
        hvc_component &l = out.layout[i];
        l.stride = l.blocks_w > 0 ? (size_t)l.blocks_w * n : 0;
        l.plane_offset = at;
        if (l.blocks_w > 0 && l.blocks_h > 0) at += (size_t)l.blocks_w * n * (size_t)l.blocks_h * n;
    }
    out.pixel_bytes = at;
}

namespace hvc {

struct MixedPlaneK {            // 48 bytes
    unsigned long long coef_base; // int16 elements from the launch's coefficient pointer
    unsigned long long pix_base;  // bytes from the launch's pixel pointer
    unsigned long long stride;    // bytes per pixel row
    int bw, nblk;                 // blocks per block row, blocks in the plane
    unsigned magic;               // ceil(2^32 / bw), 0 for bw == 1 (CompK::magic)
    int table;                    // index of its table entry
    unsigned unit0;               // its first work unit
    unsigned dwords;              // (the scaled block stage) its first byte and its stride are multiples of 4: dword stores
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
// n = 4, 2, 1: the plan of the SCALED block stage (k_decode_mixed_scaled, hvc_mixed_scaled.hip) -- units, map and tables as
// for n = 8; .plane_offset / .stride describe planes of blocks_w * n x blocks_h * n samples, which may lie at any offset
// with any stride >= blocks_w * n (the 16-byte rule of the coefficient planes stays); a descriptor's `dwords` is set when
// pix_addr (the address pixel offsets count from: only its low bits matter) + pix_base and the stride are multiples of 4.
int mixed_plan_build(const hvc_jpeg_info *infos, const size_t *coef_offsets, const size_t *pixel_offsets, const int *frames,
                     int n_list, MixedPlan &plan, int n = 8, uintptr_t pix_addr = 0);

// The tables of a plan in the form the libjpeg-exact block stage wants (k_islow_mixed, hvc_mixed_libjpeg.hip; IslowParams::qq's
// form): one record of HVC_ISLOW_PAIR_WORDS dwords per table of plan.tables, in that order, dword i = q[2i] | q[2i+1] << 16
// in zig-zag order with all 16 bits of every entry.  An array of its own beside the plan's three: MixedTableK and
// everything k_decode_mixed reads stay what they are.  An empty plan gives no record.
#define HVC_ISLOW_PAIR_WORDS 32
void mixed_islow_pairs_build(const MixedPlan &plan, std::vector<unsigned> &pairs);

// hvc_jpeg_mixed_layout of include/hvc_jpeg.h
int mixed_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, size_t align, hvc_jpeg_info *infos, int *status,
                 size_t *pixel_offsets, size_t *total_bytes);
// hvc_jpeg_mixed_scaled_layout of include/hvc_jpeg.h
int mixed_scaled_layout(const uint8_t *const *jpegs, const size_t *sizes, int n_files, int scale_denom, size_t align, hvc_jpeg_info *infos,
                        hvc_jpeg_info *scaled, int *status, size_t *pixel_offsets, size_t *total_bytes);

} // namespace hvc
#endif
