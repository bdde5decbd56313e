// hvc_mixed_decode_chunks.h -- how a MIXED DECODE batch of files is cut into chunks (internal), for decode_batch_mixed_impl
// (hvc_capi_mixed.hip) in all its forms and with either Huffman reader: which files take part, where every file's records
// lie in its chunk's ring slots, what the slots have to hold, and which bytes of a chunk's output slot go back to host memory.
// Plain C++, no HIP: the stand-alone program tests/host_harness/mixed_decode_chunks_harness.cpp runs it under sanitizers.
#ifndef HVC_MIXED_DECODE_CHUNKS_H
#define HVC_MIXED_DECODE_CHUNKS_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/hvc_jpeg.h"
#include "hvc_resize_plan.h"

// What the files of a mixed batch become.  Default: their padded planes, at pixel_offsets.  rgb_offsets set: RGB images
// there (`pixels` / `pixel_cap` are the RGB buffer), rows rgb_row_strides[f] apart (nullptr, or an entry of 0: tight), through
// k_ycc_to_rgb_mixed behind every chunk's block stage; the planes stay in a device ring.
// scale_denom 2, 4, 8: the planes (or the planes the images are made of) are those of hvc_jpeg_scaled_info, through
// k_decode_mixed_scaled; `infos` stay the FULL-size infos, the chunk plan derives the scaled ones.
// out_widths set (with rgb_offsets): the RGB images go to a device ring slot of their own, tight, and the two resampling passes
// (hvc_capi_resize.hip) take image f from there to out_widths[f] x out_heights[f] at rgb_offsets[f], rows rgb_row_strides[f] apart.
struct MixedForm {
    const size_t *rgb_offsets = nullptr, *rgb_row_strides = nullptr;
    int layout = 0;
    int scale_denom = 1;
    const int *out_widths = nullptr, *out_heights = nullptr;
    int filter = 0;
    // (resized form) hvc_resize_opts: a box (4 singles) and a mirror flag per file, nullptr: none; out_elem 2 / 4: a file's record
    // is its image in elements of that many bytes, looked up in `lut` (host memory, 3 * 256 elements) by the vertical pass
    const float *boxes = nullptr;
    const uint8_t *mirror = nullptr;
    int out_elem = 0;
    const void *lut = nullptr;
    size_t elem() const { return out_elem ? (size_t)out_elem : 1; }
    bool rgb() const { return rgb_offsets != nullptr; }
    bool resized() const { return rgb() && out_widths != nullptr; }
};

namespace hvc {

struct MixedDecodeChunk {
    int first = 0, count = 0;            // positions in `take`
    size_t coef_bytes = 0;               // its files' coefficient records, one after another
    size_t pix_lo = 0, pix_hi = 0;       // the bytes of `pixels` its files cover (pix_lo on 8; both 0: no output byte)
    size_t plane_bytes = 0;              // (RGB forms) its files' padded planes, each on 64 bytes
    size_t rgb_bytes = 0, mid_bytes = 0; // (resized form) its files' tight RGB images at decoded size, the passes' intermediates
};

struct MixedDecodeChunks {
    std::vector<int> take;     // the files that take part, in order
    std::vector<int> chunk_of; // per file: its chunk, -1 = left out
    std::vector<MixedDecodeChunk> chunks;
    std::vector<int> chunk_first, chunk_count; // first / count of every chunk (what MixedGpuReader::begin is given)
    // per file: the coefficient record from the start of its chunk's slot (int16 elements); its record in `pixels` from its
    // chunk's pix_lo (bytes; host output only, else 0) and that record's bytes (its planes, or the span of its image)
    std::vector<size_t> coef_rel, pix_rel, out_bytes;
    // RGB forms, else empty: the padded planes in the chunk's plane slot (bytes, on 64), the tight row of the file's record in
    // `pixels` and its rows (mixed_rgb_row_bytes / mixed_rgb_rows of the image's size, resized: of the size the caller names)
    std::vector<size_t> plane_rel, row_bytes, rows;
    // resized form, else empty: the tight image at decoded size in the chunk's RGB slot (bytes, on 64) and the image as the
    // resampling plan wants it, from that slot to dst_offset = pix_rel[f] (host output) or pixel_offsets[f] (device output)
    std::vector<size_t> rgb_rel;
    std::vector<ResizeImage> rimg;
    // scale_denom 2, 4, 8, else empty: hvc_jpeg_scaled_info of every file that reached the cut (what describes its OUTPUT: its
    // planes, its image's size -- blocks, tables and coefficient offsets are the full-size info's)
    std::vector<hvc_jpeg_info> scaled;
    const hvc_jpeg_info *out_infos(const hvc_jpeg_info *infos) const { return scaled.empty() ? infos : scaled.data(); }
    // what a ring slot has to hold, the maximum over the chunks: coefficients (coef_bytes), output (pix_hi - pix_lo; host output
    // only, else 0), planes, RGB images, intermediates
    size_t coef_ring = 0, out_ring = 0, plane_ring = 0, rgb_ring = 0, mid_ring = 0;
    int largest = 0; // files of the fullest chunk
};

// The form first.  HVC_E_INVALID_ARG for the call: a scale_denom that is not 1, 2, 4 or 8; under the resized form (and a set
// that holds a file) no out_heights beside out_widths, or a filter that is none of HVC_RESIZE_BOX / BILINEAR / BICUBIC.
//
// Then the files with status[f] == HVC_OK, in order, cut into chunks by the bytes of their coefficient records (coef_count
// int16 elements): a chunk that holds a file closes when the next record would take it past chunk_bytes (0: 64 MiB), so a file
// above chunk_bytes has a chunk of its own.  Every other file keeps the status it came with and is skipped.
// A file's record in `pixels` (out_bytes): its planes (pixel_bytes of its info, or of the scaled info), or under an RGB form
// mixed_rgb_span of its image -- the decoded (scaled) size, or under the resized form the size the caller names -- with rows
// rgb_row_strides[f] apart (nullptr, or an entry of 0: tight).
// The file's own result, written to status[f] (it is left out and stops nobody else): under an RGB form a sampling that
// rgb_sampling_of does not know (HVC_E_INVALID_ARG); under the resized form what resize_image_status_box answers for its image,
// its box (in the coordinates of the image at decoded size) and its mirror flag, and a row stride below the tight output row
// (HVC_E_INVALID_ARG).  Under a typed output (out_elem 2 / 4) the tight row, the record and the copies back are those of
// out_elem bytes per sample.
// HVC_E_INVALID_ARG for the call: a null jpegs[f] or an n_comp outside 0 .. 4 of a file that takes part; under an RGB form a
// negative image size or (not resized) a row stride below the tight row; a record of bytes that starts beyond pixel_cap or
// ends beyond it (ending exactly at pixel_cap is fine); after the loop, a record of bytes anywhere and have_pixels false.
// HVC_E_ALIGNMENT for the call: full-size planes of bytes at a pixel offset that is no multiple of 8 (scaled planes and
// images lie at any offset).  Statuses written before the file that ends the call stay.
// In a chunk: coef_rel is the running sum of the records before the file; pix_lo the smallest pixel offset of its files with
// output bytes, rounded DOWN to 8 (the slot keeps every offset modulo 8), pix_hi the largest end; plane_rel the running sum of
// the (scaled) infos' pixel_bytes, each rounded up to 64; rgb_rel the same over the tight images at decoded size; mid_bytes adds
// per file 64 + (tight output-width row rounded up to 4) * decoded height * planes (3 planar, 1 interleaved), an upper bound of
// what resize_plan_build wants.  pix_rel = pixel_offsets[f] - pix_lo for host output (where == HVC_MEM_HOST) and a record of
// bytes, else 0.  No file taking part: HVC_OK and an empty plan.
int mixed_decode_chunks_build(const hvc_jpeg_info *infos, int *status, const uint8_t *const *jpegs, const size_t *pixel_offsets,
                              size_t pixel_cap, bool have_pixels, int n_files, size_t chunk_bytes, int where, const MixedForm &form,
                              MixedDecodeChunks &plan);

// One copy of a chunk's output slot back to host memory, in bytes from the slot's start (= from pix_lo in `pixels`): rows == 0:
// `bytes` bytes at lo; else `rows` rows of row_bytes bytes, row_stride apart on both sides, the first at lo.
struct MixedDecodeRun {
    size_t lo = 0, bytes = 0;
    size_t row_stride = 0, row_bytes = 0, rows = 0;
};
// The copies of chunk k, in order (host output).  A file is skipped -- no copy touches its record -- when status[f] is not
// HVC_OK, when it has no output bytes, or when back[f] is set (back may be nullptr: the GPU reader handed the file to the host
// reader, whose pass writes it).  The records of consecutive good files go back in one copy where only alignment padding lies
// between them: a file joins the current run if it is the next position in `take` after the run's last file, starts at or
// after the run's end, and the gap is below 4096 bytes -- below 1 byte, so only records that touch, when `scaled` (records at
// any offset: no byte between them is anybody's), under the resized form, or host_reader_only (what lies between two of that
// pass's files may be the record of a file masked out of it).  Else the run ends and the file starts the next.  Under an RGB
// form a file whose row stride is above its tight row ends the run and is one 2-D copy of its rows: the caller's bytes between
// rows stay; the file after it starts a new run.
void mixed_decode_download_runs(const MixedDecodeChunks &plan, int k, const int *status, const char *back, const MixedForm &form,
                                bool scaled, bool host_reader_only, std::vector<MixedDecodeRun> &runs);

} // namespace hvc
#endif
