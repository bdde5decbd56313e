// hvc_huff_mixed_plan.h -- the host plan of the MIXED GPU Huffman coder (internal): coefficient records of frames of
// different geometry behind one chain of launches of hvc_huff_mixed.hip.  Plain C++, no device code:
// hvc_huff_mixed_plan.cpp builds what the kernels read from device memory, and the stand-alone program
// tests/host_harness/huff_mixed_plan_harness.cpp runs it under sanitizers.
//
//   file descriptors   one per frame the coder takes, in list order: its MCU grid and where its lengths and its bit buffer
//                      start in the chunk's scratch.  File k's counters (bits, bytes, pieces, 0xFF bytes), status word,
//                      symbol counts, code tables and specs are entry k of arrays the launch names.
//   plane descriptors  three per file: the plane in blocks, its sampling factors, its table set, its record, its file
//   unit map           one plane index per work unit; a unit = 64 consecutive blocks of ONE plane = one wavefront
//                      (HVC_MIXED_UNIT, HVC_MIXED_GROUP units per workgroup, as k_encode_mixed / k_decode_mixed)
// The pieces (64 bytes of a file's unstuffed segment) have no map: how many a file has is known on the device only, after the
// length pass, and the piece kernels find their file by a search over the files' piece bases (hvc_huff_mixed.hip says why).
// Sizing: a file's bit buffer is what huffman_prepare gives a frame of a uniform batch -- 216 bytes per coded block (64
// fields of 27 bits) + 8, rounded up to 64-byte pieces.  Nothing tighter is known without a host round trip behind the
// length pass.  Every file's buffer starts on a piece, so no word is shared between files.
#ifndef HVC_HUFF_MIXED_PLAN_H
#define HVC_HUFF_MIXED_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/hvc_jpeg.h"
#include "hvc_mixed_plan.h" /* HVC_MIXED_UNIT, HVC_MIXED_GROUP, HVC_MIXED_MAX_UNITS */

#define HVC_HUFF_MIXED_MAX_FILES 65535 /* k_huff_build's grid: one row per file */

namespace hvc {

struct HuffMixedFileK {             // 40 bytes
    int mbs_wide, mbs_high, blocks_per_mcu;
    unsigned blocks;                // coded blocks = mbs_wide * mbs_high * blocks_per_mcu
    unsigned long long lens_base;   // its first entry of the lengths (scan order)
    unsigned long long bitbuf_base; // its first 32-bit word of the bit buffer (a multiple of 16: a piece)
    unsigned bitbuf_words;          // the words it owns there (a multiple of 16)
    unsigned pad;
};
static_assert(sizeof(HuffMixedFileK) == 40, "HuffMixedFileK");

struct HuffMixedPlaneK {            // 48 bytes
    unsigned long long coef_base;   // int16 elements from the launch's coefficient pointer (a multiple of 8)
    int bw, nblk;                   // blocks per block row, blocks in the plane
    int h, v;                       // sampling factors = blocks per MCU in x / y
    int mcu_base;                   // index of the component's first block inside an MCU
    int table;                      // 0 = luma tables, 1 = chroma tables
    unsigned unit0;                 // its first work unit
    unsigned file;                  // index of its file descriptor
    unsigned pad[2];
};
static_assert(sizeof(HuffMixedPlaneK) == 48, "HuffMixedPlaneK");

struct HuffMixedPlan {
    std::vector<HuffMixedFileK> files;   // the frames taken, in list order
    std::vector<int> file_of;            // ... and which frame of the set each of them is
    std::vector<int> status;             // [n_list] the code of every listed frame: HVC_OK = taken
    std::vector<HuffMixedPlaneK> planes; // three per file
    std::vector<unsigned> map;           // unit -> plane
    unsigned long long lens_total = 0;   // entries of the lengths
    unsigned long long bitbuf_words = 0; // words of the bit buffer
    unsigned long long pieces_cap = 0;   // bitbuf_words / 16: the most pieces the chunk can have (the piece counts' entries)
    unsigned long long coef_elems = 0;   // coefficients of the files taken (what a segment slot is sized from)
};

// The geometry of one frame, or why the coder cannot take it (`k`: everything but the bases):
//   hvc_jpeg_encoder_check's code (which covers n_comp != 3); HVC_E_INVALID_ARG: a component without a block, no coded block
//   at all, or -- optimised -- all components on one table set (as hvc_huffman_optimal_tables); HVC_E_TOO_LARGE: 32-bit bit
//   offsets exceeded (huffman_prepare's bound); HVC_E_ALIGNMENT: a coefficient plane not on 16 bytes
int huff_mixed_geometry(const hvc_jpeg_info &info, bool optimised, HuffMixedFileK &k, HuffMixedPlaneK (&planes)[3]);

// The plan of frames[0 .. n_list) of the set (nullptr: 0 .. n_list - 1), frame f's record at coef_offsets[f] (int16
// elements).  Never fails for a frame's sake: a frame the coder cannot take has its code in plan.status and is left out.
// For the call's sake: HVC_E_INVALID_ARG (null arguments, a list entry below 0), HVC_E_TOO_LARGE (more than
// HVC_HUFF_MIXED_MAX_FILES files taken, HVC_MIXED_MAX_UNITS units or 2^32 - 1 pieces); the plan is empty then.
int huff_mixed_plan_build(const hvc_jpeg_info *infos, const size_t *coef_offsets, const int *frames, int n_list, bool optimised,
                          HuffMixedPlan &plan);

// The hand-back decision of a chunk.  offsets[0 .. n_files]: the packed segments' offsets as the coder made them;
// file_status[k]: file k's status word (non-zero = flagged: it holds no bytes); capacity: the bytes of the segment slot.
// complete: the files whose segments lie inside the slot; handed_back: every file from the first whose segment ends past the
// capacity, and every flagged file.  Both in file order; together they name every file once.
void huff_mixed_hand_back(const unsigned long long *offsets, const unsigned *file_status, int n_files, unsigned long long capacity,
                          std::vector<int> &complete, std::vector<int> &handed_back);

} // namespace hvc
#endif
