// hvc_mixed_encode_chunks.h -- how a MIXED ENCODE batch of files is cut into chunks (internal), for both file pipelines:
// encode_batch_mixed_impl (hvc_capi_mixed_encode.hip, the host coder) and encode_batch_mixed_gpu_impl (hvc_capi_mixed_coder.hip,
// the GPU coder, which hands files back to the first: their chunks have to be the same).  With it the host-only parts of the
// padding workers.  Plain C++, no HIP: the stand-alone program tests/host_harness/mixed_encode_chunks_harness.cpp runs it
// under sanitizers.
#ifndef HVC_MIXED_ENCODE_CHUNKS_H
#define HVC_MIXED_ENCODE_CHUNKS_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/hvc_jpeg.h"

// What frames[f] of a mixed encode batch is.  Default: a raw planar frame (tight Y, U, V).  rgb: an RGB image of `layout`
// with rows rgb_row_strides[f] apart (nullptr, or an entry of 0: tight); the padding workers copy its rows tight into the
// pinned ring, the chunk goes up into a device RGB slot and k_rgb_to_ycc_mixed writes the chunk's zeroed plane slot from it in
// front of k_encode_mixed.  Chunks, records and everything behind the block stage are the same.
struct MixedEncodeInput {
    bool rgb = false;
    int layout = 0;
    const size_t *rgb_row_strides = nullptr;
};
// the RGB input form's host parts: the frame's own status (HVC_E_INVALID_ARG: an odd size under its sampling, a row stride
// below the row), the bytes of its tight image, its rows into the pinned slot
int encode_rgb_frame_status(const hvc_jpeg_info &info, const MixedEncodeInput &in, int f);
size_t encode_rgb_frame_bytes(const hvc_jpeg_info &info, const MixedEncodeInput &in);
void encode_rgb_frame_copy(const hvc_jpeg_info &info, const MixedEncodeInput &in, int f, const uint8_t *src, uint8_t *dst);
// Plane.blit_available of a raw planar frame (tight Y, U, V of the info's actual sizes) into the zero-padded planes of `rec`
void pad_frame(const hvc_jpeg_info &info, const uint8_t *src, uint8_t *rec);
// what a frame's records cover: bytes of pixels, elements of coefficients
void encode_frame_spans(const hvc_jpeg_info &fi, size_t &pixel_span, size_t &coef_span);

namespace hvc {

struct MixedEncodeChunk {
    int first = 0, count = 0; // positions in `take`
    size_t pix_bytes = 0, coef_elems = 0, rgb_bytes = 0;
};

struct MixedEncodeChunks {
    std::vector<int> take;     // the frames that take part, in order
    std::vector<int> chunk_of; // per frame: its chunk, -1 = left out
    std::vector<MixedEncodeChunk> chunks;
    // per frame, from the start of its chunk's slot: the padded pixel record (bytes, on 64), the coefficient record (int16
    // elements, on 32), the tight RGB image (bytes, on 64; RGB input only, else empty)
    std::vector<size_t> pix_rel, coef_rel, rgb_rel;
    // what a ring slot has to hold: pixels or images in (eh_in: the pinned images; ed_in: the planes), coefficients out, images
    size_t in_bytes = 0, out_bytes = 0, rgb_bytes = 0;
    int largest = 0;         // files of the fullest chunk
    uint64_t coef_total = 0; // bytes of all chunks' coefficient records
};

// The frames with status[f] == HVC_OK, cut into chunks by the bytes of their padded pixel records: a chunk that holds a frame
// closes when the next record would take it past chunk_bytes (0: 64 MiB) or when it holds max_files_per_chunk files (0: no
// cap), so a frame above chunk_bytes has a chunk of its own.  A frame the block stage, the coder or the padding workers would
// refuse -- hvc_jpeg_encoder_check, a one-frame mixed_encode_plan_build, a record of no bytes, planes that are not 8 * blocks,
// encode_rgb_frame_status under RGB input -- gets that code in status[f] and is left out.  HVC_E_INVALID_ARG for the call: a
// null frames[f] or jpegs[f] of a frame that takes part, records that span more than the info says (not a record of the
// layout call); statuses written before that frame stay.
int mixed_encode_chunks_build(const hvc_jpeg_info *infos, int *status, const uint8_t *const *frames, uint8_t *const *jpegs, int n_frames,
                              size_t chunk_bytes, const MixedEncodeInput &in, int max_files_per_chunk, MixedEncodeChunks &plan);

} // namespace hvc
#endif
