// hvc_hdec_mixed_plan.h -- the host plan of the MIXED GPU Huffman reader (internal): files of different geometry, size and
// Huffman tables behind one chain of launches of hvc_hdec_mixed.hip.  Plain C++, no device code: hvc_hdec_mixed_plan.cpp
// builds what the kernels read from device memory, and the stand-alone program tests/host_harness/hdec_mixed_plan_harness.cpp
// runs it under sanitizers.
//
//   file descriptors   one per file the reader takes, in list order: where its segment, its subsequences, its work units,
//                      its coefficient record and its DC-difference row start, and its geometry (what HdParams carries as
//                      kernel arguments for a uniform batch)
//   table records      the DISTINCT Huffman table sets of those files (deduplicated by content): the plan names, per
//                      record, the file whose tables it holds; the caller converts them (make_frame_tabs)
//   unit map           one file index per work unit; a unit = 64 consecutive subsequences of ONE file = one wavefront, so
//                      that everything a wavefront looks up about its file is wave-uniform
#ifndef HVC_HDEC_MIXED_PLAN_H
#define HVC_HDEC_MIXED_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/hvc_jpeg.h"
#include "hvc_hdec.h"

#define HVC_HDM_UNIT 64  /* subsequences per work unit = lanes per wavefront */
#define HVC_HDM_GROUP 4  /* units per workgroup */

namespace hvc {

struct HdmFileK {                 // 192 bytes: 48 dwords, a wavefront copies it to LDS with one load per lane
    unsigned ecs_off;             // bytes from the chunk's segment buffer (a multiple of the subsequence's bytes)
    unsigned sub0, n_sub;         // its first subsequence in the chunk, how many it has (the zero one behind its bytes included)
    unsigned unit0;               // its first work unit
    unsigned long long coef_base; // int16 elements from the launch's coefficient pointer (a multiple of 8)
    unsigned need;                // blocks the file must have: MCUs x blocks per MCU
    unsigned blocks_per_mcu, mbs_wide, n_comp;
    unsigned selmask;             // 2 bits per block b of an MCU: its component (whose tables it reads)
    unsigned tabrec;              // index of its table record
    unsigned dcd0;                // first entry of its DC-difference row (`need` entries, scan order)
    unsigned pad[3];
    unsigned h[4], v[4], bw[4], mcu_base[4], coef_off[4]; // per component (coef_off: int16 elements inside the record)
    unsigned char b2comp[HVC_HD_MAX_MCU_BLOCKS], b2sx[HVC_HD_MAX_MCU_BLOCKS], b2sy[HVC_HD_MAX_MCU_BLOCKS];
};
static_assert(sizeof(HdmFileK) == 192, "HdmFileK: 48 dwords");

// why a file is not in the plan
enum HdmRefusal {
    HDM_TAKEN = 0,
    HDM_NO_COMPONENTS = 1, // n_comp outside 1..3, or a sampling factor below 1
    HDM_MCU_BLOCKS = 2,    // more than HVC_HD_MAX_MCU_BLOCKS blocks per MCU
    HDM_MCU_GRID = 3,      // the MCU grid leaves a plane (the model raises: the host reader decides)
    HDM_TOO_LARGE = 4,     // sizes beyond the 32-bit indices (of the file, or the chunk with it in)
    HDM_TABLES = 5,        // tables that are no prefix code (or anything else the segment's preparation refused)
    HDM_NO_BLOCKS = 6,     // a file without a block: nothing to read
    HDM_PLACE = 7,         // a coefficient record that is not on 16 bytes, a segment that is not on a subsequence boundary
};

// one file as the plan sees it
struct HdmFileIn {
    const hvc_jpeg_info *info;
    size_t ecs_off;          // where the caller put its segment in the chunk's segment buffer (a subsequence boundary)
    size_t seg_bytes;        // bytes of its unstuffed segment; hdm_file_room(seg_bytes) bytes from ecs_off on are the file's
    const HdTables *tables;  // as prepare_gpu_decode_to made them
    bool tables_ok;          // prepare_gpu_decode_to's gpu_ok
    size_t coef_base;        // int16 elements from the launch's coefficient pointer
    int tabrec = -1;         // >= 0: the caller has found the file's table record already (its index; files that share one carry
                             // the same tables); -1: the plan finds it by content
};

struct HdmPlan {
    std::vector<HdmFileK> files;      // the files taken, in list order
    std::vector<int> file_of;         // ... and which entry of the input each of them is
    std::vector<int> refusal;         // [n_list] HdmRefusal of every listed file
    std::vector<int> tab_src;         // per table record: the input entry whose tables it holds
    std::vector<unsigned> map;        // unit -> index into `files`
    unsigned total_sub = 0;           // subsequences of the chunk
    size_t seg_bytes = 0;             // the segment buffer: up to the end of the last file's room (HVC_HD_ECS_SLACK comes behind)
    size_t dcd_entries = 0;           // the DC-difference rows
};

// subsequences of a file whose segment has `seg_bytes` bytes: its own and one of zeros
inline size_t hdm_file_subs(size_t seg_bytes) { return (seg_bytes + HVC_HD_SUBSEQ_BITS / 8 - 1) / (HVC_HD_SUBSEQ_BITS / 8) + 1; }
// ... and the room they take in the segment buffer (16 bytes of overshoot behind them; a multiple of the subsequence's bytes)
inline size_t hdm_file_room(size_t seg_bytes) { return (hdm_file_subs(seg_bytes) + 1) * (HVC_HD_SUBSEQ_BITS / 8); }

// The geometry of one file (what gd_geometry of hvc_capi_reader.hip derives for a uniform batch), or why the GPU reader
// cannot take it.  Fills everything of `k` that does not depend on the file's place in a chunk.
int hdm_geometry(const hvc_jpeg_info &info, HdmFileK &k);

// The plan of files[list[0 .. n_list)] (list == nullptr: 0 .. n_list - 1), in that order.  Never fails for a file's sake: a
// file the reader cannot take is named in plan.refusal and left out.  HVC_E_INVALID_ARG: a list entry outside [0, n_files),
// a null info or table pointer.
int hdm_plan_build(const HdmFileIn *files, int n_files, const int *list, int n_list, HdmPlan &plan);

} // namespace hvc
#endif
