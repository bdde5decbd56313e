// hvc_huff_mixed.h -- parameter block of the MIXED GPU Huffman coder (internal; hvc_huff_mixed.hip).
#ifndef HVC_HUFF_MIXED_H
#define HVC_HUFF_MIXED_H

#include <hip/hip_runtime.h>

#include "hvc_huff.h"
#include "hvc_huff_mixed_plan.h"

namespace hvc {

struct HuffMixedParams {
    const int16_t *coefs;            // the launch's coefficient pointer (the planes' coef_base count from it)
    const HuffMixedFileK *files;     // device: [n_files]
    const HuffMixedPlaneK *planes;   // device: [3 n_files]
    const unsigned *map;             // device: [n_units] unit -> plane
    unsigned n_files, n_units;
    const unsigned *tables;          // device: [2][16 dc + 256 ac]; file k's at tables + k * table_stride
    size_t table_stride;             // 0: the default tables for every file; HUFF_TABLE_WORDS: per file (optimised)
    // optimised tables (hist != nullptr): k_hm_hist counts into hist, k_huff_build writes opt_tables (== tables) and specs
    unsigned *hist;                  // [n_files][2][16 + 256]
    unsigned *opt_tables;            // [n_files][2][16 + 256]
    hvc_huff_spec *specs;            // [n_files][4]
    unsigned *lens;                  // [lens_total]: bit lengths in scan order per file, then offsets
    unsigned *file_bits, *file_bytes, *file_pieces, *file_ff; // [n_files]
    unsigned *file_status;           // [n_files]: bit 0 a value without a code (HVC_E_RANGE), bit 1 buffer too small (cannot happen)
    unsigned *piece_base;            // [n_files + 1]: exclusive scan of file_pieces: file k's first piece among the chunk's
    unsigned *bitbuf;                // [bitbuf_words]
    unsigned long long bitbuf_words;
    unsigned *ff;                    // [pieces_cap]: 0xFF bytes per piece (indexed as piece_base says), then offsets inside the file
    unsigned pieces_cap;
    unsigned long long *out_offsets; // [n_files + 1]
    uint8_t *out;
    unsigned long long out_cap;
    int partial;                     // out too small: 0 = nothing is written; 1 = the files whose segments end inside out_cap are
    unsigned *status;               // one word for the launch: bit 2 = out too small
};

// The passes over P (hvc_huff_mixed.hip); the memsets of the status words, the counts and the bit buffer included.
hipError_t launch_huffman_encode_mixed(const HuffMixedParams &P, hipStream_t s);

} // namespace hvc
#endif
