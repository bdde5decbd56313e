// hvc_huff.h -- parameter block of the GPU Huffman coder (internal).
#ifndef HVC_HUFF_H
#define HVC_HUFF_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/hvc_jpeg.h"

namespace hvc {

struct HuffComp {
    int bw, bh, nblk;  // the component's coefficient plane in blocks
    int tile0;         // first workgroup tile (256 blocks) of this component inside a frame
    int h, v;          // sampling factors = blocks per MCU in x / y
    int mcu_base;      // index of this component's first block inside an MCU
    int table;         // 0 = luma tables, 1 = chroma tables (Parameters.c4xx, encoder.ml:306-349)
    size_t coef_off;   // int16 elements from the frame's coefficient record
};

struct HuffParams {
    const int16_t *coefs;
    size_t coef_fs;        // int16 elements between frames
    int n_frames, tiles_per_frame;
    int mbs_wide, mbs_high, blocks_per_mcu;
    unsigned blocks_per_frame;   // coded blocks = mbs_wide * mbs_high * blocks_per_mcu
    HuffComp comp[3];
    const unsigned *tables;      // device: [2][16 dc + 256 ac], (code << 5) | length; frame f's at tables + f * table_stride
    size_t table_stride;         // 0: one pair for every frame (the default tables); HUFF_TABLE_WORDS: per frame (optimised)
    // optimised tables (hist != nullptr): k_huff_hist counts into hist, k_huff_build writes opt_tables (== tables) and specs
    unsigned *hist;              // [n_frames][2][16 dc + 256 ac] symbol counts
    unsigned *opt_tables;        // [n_frames][2][16 + 256]
    hvc_huff_spec *specs;        // [n_frames][4]: DC0, DC1, AC0, AC1
    unsigned *lens;              // [n_frames][blocks_per_frame]: bit lengths in scan order, then offsets
    unsigned *frame_bits, *frame_bytes, *frame_pieces, *frame_ff;   // [n_frames]
    unsigned *bitbuf;            // [n_frames][bitbuf_words]: unstuffed segments, big-endian bit order
    size_t bitbuf_words;         // per frame, a multiple of 16 (64-byte pieces)
    unsigned *ff;                // [n_frames][ff_stride]: 0xFF bytes per piece, then offsets
    size_t ff_stride;
    unsigned long long *out_offsets;  // [n_frames + 1]
    uint8_t *out;
    unsigned long long out_cap;
    unsigned *status;            // bit 0: value without a code (HVC_E_RANGE); bit 2: out too small
    // restart intervals (hvc_set_restart_interval; 0 = none, and nothing below is read)
    int restart;                 // Ri: MCUs per interval
    unsigned n_intervals;        // per frame: ceil(MCUs / Ri)
    unsigned *ivl;               // [n_frames][n_intervals]: bytes per interval, then their byte bases in the unstuffed segment
};

constexpr size_t HUFF_TABLE_WORDS = 2 * (16 + 256); // one frame's two table sets

// P.hist != nullptr: the frames' own tables first (k_huff_hist, k_huff_build), then the coder's passes with them.
// P.restart > 0: the *_rst instantiations of the passes, plus k_ivl_bytes and one more scan (hvc_huff.hip)
hipError_t launch_huffman_encode(const HuffParams &P, hipStream_t s);
// k_huff_build over P.n_frames (frame, table) rows of P.hist -> P.opt_tables, P.specs; nothing else of P is read
hipError_t launch_huffman_build(const HuffParams &P, hipStream_t s);

// hvc_entropy.cpp
void default_enc_tables(uint32_t (*out)[16 + 256]);
// restart: the restart interval in MCUs (hvc_set_restart_interval), 0 = none
int optimal_specs(const ::hvc_jpeg_info *info, const int16_t *coefs, hvc_huff_spec *out, int restart = 0);
int entropy_encode_file(const ::hvc_jpeg_info *info, const hvc_huff_spec *specs, const int16_t *coefs, uint8_t *out, size_t cap,
                        size_t *out_len, int restart = 0);
int entropy_encode_optimised(const ::hvc_jpeg_info *info, const int16_t *coefs, uint8_t *out, size_t cap, size_t *out_len,
                             int restart = 0);
// specs: the four DHT bodies (DC0, DC1, AC0, AC1), nullptr = the default tables
void jpeg_header_bytes(const ::hvc_jpeg_info *info, std::vector<uint8_t> &o, const hvc_huff_spec *specs = nullptr, int restart = 0);

}
#endif
