// hvc_mixed_rgb.hip -- the colour pass over images of DIFFERENT size and sampling in one launch: planes -> RGB
// (k_ycc_to_rgb_mixed) and, under the same decomposition, RGB -> the encoder's planes (k_rgb_to_ycc_mixed, below it).
//
// k_ycc_to_rgb (hvc_rgb.hip) takes one RgbOp: one w, h and sampling in the kernarg segment, frames on blockIdx.y.  Here the
// decomposition comes from device memory (hvc_mixed_rgb_plan.h): hvc_mixed_dev.h says how (the image passes: work map, image
// descriptor, one wavefront per work unit, a wave-uniform branch on the sampling).  No LDS.
//
// Per lane: what a lane of k_ycc_to_rgb does, by the same code (HVC_YCC_LANE_TO_RGB, hvc_rgb_dev.h): 8 columns of one image
// row (4:2:0: two), chroma supersampled in registers with the ceil-window clamping, ycc4_to_rgb, 8-byte stores where the
// image's vec_* flags allow them and the bounds-checked byte path otherwise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hvc_jpeg.h"
#include "hvc_mixed_dev.h"
#include "hvc_mixed_rgb.h"
#include "hvc_rgb_dev.h"

namespace hvc {
namespace {

struct YccToRgbLane {
    template <int S, int PLANAR>
    static __device__ __forceinline__ void lane(const RgbOp &P, unsigned lr, unsigned g) {
        const size_t f = 0; // one image per RgbOp
        HVC_YCC_LANE_TO_RGB(P, f, lr, g);
    }
};

template <int PLANAR>
__global__ __launch_bounds__(HVC_MIXED_LANES) void k_ycc_to_rgb_mixed(MixedRgbParams P) {
    const MixedWave W = mixed_wave_plain();
    if (W.unit >= P.n_units) return;
    const MixedRgbImageK K = P.images[P.map[W.unit]]; // wave-uniform: read once, before any store
    MixedImageLane L;
    if (!mixed_image_lane(K, W.unit, W.lane, L)) return;
    mixed_rgb_dispatch<YccToRgbLane, PLANAR>(K.sampling, mixed_rgb_op(P, K), L.row, L.group);
}

// The way back (RGB -> the encoder's planes), under the same decomposition: P.rgb is read, the planes at P.yuv are written.
// Lanes per image: ceil(w / 8) per lane row, h lane rows (4:2:0: h / 2 -- encoding takes even sizes only, the plan checks),
// chroma rows of w / 2 samples (4:4:4: w).  Per lane: what a lane of k_rgb_to_ycc does, by the same code
// (HVC_RGB_LANE_TO_YCC): only the image's own samples are written, the padding of its planes stays what it was.
template <int S, int PLANAR>
__device__ __forceinline__ void mixed_ycc_lane(const RgbOp &P, unsigned lr, unsigned g) {
    const size_t f = 0; // one image per RgbOp
    HVC_RGB_LANE_TO_YCC(P, f, lr, g);
}

template <int PLANAR>
__global__ __launch_bounds__(HVC_MIXED_LANES) void k_rgb_to_ycc_mixed(MixedRgbParams P) {
    const unsigned lane = threadIdx.x & (HVC_MIXED_UNIT - 1);
    const unsigned unit = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * HVC_MIXED_GROUP + (threadIdx.x >> 6)));
    if (unit >= P.n_units) return; // (the whole wavefront: the last group's spare units)
    const MixedRgbImageK K = P.images[P.map[unit]]; // wave-uniform: read once, before any store
    const unsigned t = (unit - K.unit0) * HVC_MIXED_UNIT + lane;
    if (t >= K.lanes) return;
    const unsigned lr = K.groups == 1 ? t : __umulhi(t, K.magic), g = t - lr * K.groups;
    RgbOp R; // the image as k_rgb_to_ycc's parameter block: one frame, its own bases
    R.y = const_cast<uint8_t *>(P.yuv) + K.y_base;
    R.cb = const_cast<uint8_t *>(P.yuv) + K.cb_base;
    R.cr = const_cast<uint8_t *>(P.yuv) + K.cr_base;
    R.rgb = P.rgb + K.rgb_base;
    R.y_stride = K.y_stride, R.cb_stride = K.cb_stride, R.cr_stride = K.cr_stride, R.yuv_fs = 0;
    R.row_stride = K.row_stride, R.plane_stride = K.plane_stride, R.frame_stride = 0;
    R.w = K.w, R.h = K.h, R.cw = K.cw, R.ch = K.ch;
    R.vec_y = K.vec_y, R.vec_c = K.vec_c, R.vec_rgb = K.vec_rgb;
    switch (K.sampling) { // wave-uniform (the plan admits these three only)
    case HVC_YUV_420: mixed_ycc_lane<420, PLANAR>(R, lr, g); break;
    case HVC_YUV_422: mixed_ycc_lane<422, PLANAR>(R, lr, g); break;
    case HVC_YUV_444: mixed_ycc_lane<444, PLANAR>(R, lr, g); break;
    default: break;
    }
}

} // namespace

hipError_t launch_rgb_to_ycc_mixed(const MixedRgbParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    return mixed_launch(P.planar ? k_rgb_to_ycc_mixed<1> : k_rgb_to_ycc_mixed<0>, P, s, k0, k1);
}

hipError_t launch_ycc_to_rgb_mixed(const MixedRgbParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    return mixed_launch(P.planar ? k_ycc_to_rgb_mixed<1> : k_ycc_to_rgb_mixed<0>, P, s, k0, k1);
}

} // namespace hvc
