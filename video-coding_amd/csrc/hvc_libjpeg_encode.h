// hvc_libjpeg_encode.h -- the kernels of hvc_set_encode_libjpeg (hvc_libjpeg_encode.hip; the encoder of include/hvc_jpeg.h
// "Encoding bit-exact to libjpeg"): parameters and launchers (internal).
#ifndef HVC_LIBJPEG_ENCODE_H
#define HVC_LIBJPEG_ENCODE_H

#include "hvc_kernels.h"
#include "hvc_libjpeg_encode_plan.h"
#include "hvc_mixed_plan.h"

namespace hvc {

// k_fdct_islow: k_encode's geometry and record layout, libjpeg's forward DCT and quantiser
struct FdctIslowParams {
    const uint8_t *pixels;
    int16_t *coefs;
    size_t coef_fs;   // int16 elements between frames
    size_t pixel_fs;  // bytes between frames
    int n_frames, n_comp, tiles_per_frame;
    int xcd_map;      // as in EncodeParams
    unsigned xcd_magic;
    CompK comp[HVC_MAX_COMP];
    // per table, natural position k: the multiplier and the rounding term of table[Zigzag.forward[k]]
    // (libjpeg_encode_tables, hvc_libjpeg_encode_plan.h)
    unsigned magic[HVC_MAX_QTABS * 64];
    unsigned half[HVC_MAX_QTABS * 64];
};
// every block of P (grid = tiles x frames, one block per lane), every block taken as real
hipError_t launch_fdct_islow(const FdctIslowParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);

// k_dummy_blocks: the dummy blocks of a frame's records after k_fdct_islow (same stream): AC 0, DC of the source block
struct DummyCompK {
    int bw, real_w, real_h, h; // plane width in blocks, its real blocks, the horizontal sampling factor
    int first;                 // dummies of the components before this one
    size_t coef_off;           // int16 elements from the frame's coefficient record
};
struct DummyBlocksParams {
    int16_t *coefs;
    size_t coef_fs;
    int n_frames, n_comp, total; // total: dummies per frame
    DummyCompK comp[HVC_MAX_COMP];
};
// The dummy geometry of n_comp planes of bw[i] x bh[i] blocks with real_w[i] x real_h[i] real ones; false where a real size is
// not inside its plane.  P.total == 0: the frame has no dummy block and nothing needs launching.
bool dummy_blocks_geometry(DummyBlocksParams &P, int n_comp, const int *bw, const int *bh, const int *real_w, const int *real_h,
                           const int *h, const size_t *coef_off);
hipError_t launch_dummy_blocks(const DummyBlocksParams &P, hipStream_t s);

// k_fdct_islow_mixed: the same block under k_encode_mixed's decomposition (a unit is 64 blocks of one plane; map, plane
// descriptor and table record come through scalar loads), for frames of different geometry and tables in one launch
struct FdctIslowMixedParams {
    const uint8_t *pixels;
    int16_t *coefs;
    const MixedPlaneK *planes;     // device
    const FdctIslowTableK *tables; // device: one record per distinct table, MixedPlaneK::table indexes it
    const unsigned *map;           // device: n_units entries
    unsigned n_units;
    int xcd_map;
    unsigned xcd_magic;
};
hipError_t launch_fdct_islow_mixed(const FdctIslowMixedParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);
// k_dummy_blocks_mixed: one lane per pair (device memory, n of them), after k_fdct_islow_mixed on the same stream
hipError_t launch_dummy_blocks_mixed(int16_t *coefs, const DummyPairK *pairs, unsigned n, hipStream_t s);

// k_rgb_to_ycc_libjpeg[_mixed]: RGB -> planes with libjpeg's chroma averaging (the lane: hvc_rgb_libjpeg_dev.h) over a plan
// whose lane grid is libjpeg_rgb_plan_lanes' (hvc_libjpeg_encode_plan.h).  pad: the replicated edge up to whole blocks.
struct RgbLibjpegParams { // uniform: one image description, n_frames frames rgb_fs / yuv_fs bytes apart
    const uint8_t *rgb;
    uint8_t *yuv;
    size_t rgb_fs, yuv_fs;
    int n_frames, planar, pad;
    MixedRgbImageK image;
};
hipError_t launch_rgb_to_ycc_libjpeg(const RgbLibjpegParams &P, hipStream_t s);
struct RgbLibjpegMixedParams {
    const uint8_t *rgb;
    uint8_t *yuv;
    const MixedRgbImageK *images; // device
    const unsigned *map;          // device: n_units entries
    unsigned n_units;
    int planar, pad;
};
hipError_t launch_rgb_to_ycc_libjpeg_mixed(const RgbLibjpegMixedParams &P, hipStream_t s, hipEvent_t k0 = nullptr, hipEvent_t k1 = nullptr);

} // namespace hvc
#endif
