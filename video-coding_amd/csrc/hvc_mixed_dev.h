// hvc_mixed_dev.h -- the decomposition of the MIXED kernels, stated once (internal): what every kernel that works on frames
// or images of DIFFERENT geometry in one launch does before and after its own arithmetic, and the one host launcher.
// Everything here has internal linkage: include it in a .hip file only.
//
// The decomposition comes from device memory (hvc_mixed_plan.h, hvc_mixed_rgb_plan.h, hvc_resize_plan.h): a work map names
// the plane (block stage) or the image (colour and resize passes) of every work unit, a descriptor says where that unit's
// data lives.  A work unit is one wavefront of ONE plane or image -- 64 consecutive blocks, or 64 consecutive lanes -- so the
// map entry, the descriptor and whatever table it names are wave-uniform: the unit number goes through readfirstlane, the
// lookups become scalar loads and live in SGPRs, exactly where the single-geometry kernels find their kernarg copies.  A
// workgroup is HVC_MIXED_GROUP consecutive units (HVC_MIXED_LANES lanes); its wavefronts share nothing and meet at no
// barrier, so a unit beyond n_units (the last group's spare units) returns as a whole wavefront.
//
//   block stage   unit -> MixedPlaneK; lane l of the unit has block b = (unit - unit0) * 64 + l of the plane, (by, bx) by
//                 the descriptor's reciprocal (bw == 1: magic is 0 and by = b).  A lane with b >= nblk is INACTIVE: it is
//                 clamped to the plane's last block, computes it and stores nothing.  The groups go over the XCDs by
//                 xcd_work (hvc_kernels.h) with gridDim.y == 1: a permutation of the groups, or the plain order.
//   image passes  unit -> MixedRgbImageK / ResizeImageK; lane t = (unit - unit0) * 64 + l of the image, (row, group) by the
//                 descriptor's reciprocal (groups == 1: row = t); a lane with t >= lanes does not exist and returns.  The
//                 vertical resize splits the UNIT, not the lane, so that a unit lies in one row (mixed_image_row_lane).
//                 Groups as dispatched.
//   forward tail  the forward block stages leave through LDS: a wavefront transposes its 64 records (8 KiB) through its own
//                 XOR-swizzled region -- 16-byte slots, lane l writes slot 8 l + (j ^ (l & 7)), conflict-free for the
//                 ds_write_b128 and for the ds_read_b128 -- and stores the unit's coefficient run, contiguous in the plane's
//                 record, as whole 1 KiB pieces; blocks at or beyond nblk are not stored.  The region is wave-private: the
//                 wave's own ds operations are ordered, no barrier.  32 KiB of LDS per group.
// k_islow_mixed, k_encode_mixed, k_fdct_islow_mixed and k_rgb_to_ycc_mixed spell this decomposition out by hand instead of
// calling the helpers below: through the helpers their registers or vector instruction counts moved
// (profiles/mixed_units_refactor.txt), so for these four the prose above is the specification and the code is theirs.
#ifndef HVC_MIXED_DEV_H
#define HVC_MIXED_DEV_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hvc_jpeg.h"
#include "hvc_kernels.h" /* xcd_work, xcd_map_for */
#include "hvc_mixed_plan.h"
#include "hvc_mixed_rgb.h"
#include "hvc_rgb_dev.h" /* RgbOp */

#define HVC_MIXED_LANES (HVC_MIXED_UNIT * HVC_MIXED_GROUP) /* lanes per workgroup, every mixed kernel */

namespace hvc {
namespace {

// ---------------------------------------------------------------------------
// The work unit of this wavefront and the lane's number in the unit
struct MixedWave {
    unsigned unit; // wave-uniform (readfirstlane); >= n_units: a spare unit of the last group
    int lane;
};
__device__ __forceinline__ MixedWave mixed_wave_of_group(unsigned group) {
    MixedWave w;
    w.lane = (int)(threadIdx.x & (HVC_MIXED_UNIT - 1));
    w.unit = (unsigned)__builtin_amdgcn_readfirstlane((int)(group * HVC_MIXED_GROUP + (threadIdx.x >> 6)));
    return w;
}
// block stage: the groups permuted over the XCDs (gridDim.y == 1; xcd_map 0: the plain order)
__device__ __forceinline__ MixedWave mixed_wave_xcd(int xcd_map, unsigned xcd_magic) {
    unsigned wf, wt;
    xcd_work(xcd_map, xcd_magic, wf, wt);
    return mixed_wave_of_group(wf * gridDim.x + wt);
}
// image passes: groups as dispatched
__device__ __forceinline__ MixedWave mixed_wave_plain() { return mixed_wave_of_group(blockIdx.x); }

// ---------------------------------------------------------------------------
// The block of a lane.  N = samples per block side in the pixel plane (8; 4, 2, 1: the scaled block stage).  bw and stride
// are wave-uniform.
template <int N, class Coef, class Pix>
struct MixedBlock {
    bool active;   // the lane has a block of its own: only then it stores
    unsigned bx;   // the block's column in its block row
    int bw;
    size_t stride;
    Coef *rec;     // the block's 64-coefficient record
    Pix *pix;      // its first sample
};
// block b of the plane -> where it is; 0 <= b < nblk is the caller's business (k_decode_mixed_wide checks an id from memory
// itself before it asks), and so is active
template <int N, class Coef, class Pix>
__device__ __forceinline__ MixedBlock<N, Coef, Pix> mixed_block_at(const MixedPlaneK &K, int b, Coef *coefs, Pix *pixels) {
    MixedBlock<N, Coef, Pix> r = {};
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    r.bx = (unsigned)b - by * (unsigned)K.bw;
    r.bw = K.bw;
    r.stride = (size_t)K.stride;
    r.rec = coefs + (size_t)K.coef_base + (size_t)b * 64;
    r.pix = pixels + (size_t)K.pix_base + (size_t)by * N * r.stride + (size_t)r.bx * N;
    return r;
}
template <int N, class Coef, class Pix>
__device__ __forceinline__ MixedBlock<N, Coef, Pix> mixed_block(const MixedPlaneK &K, unsigned unit, int lane, Coef *coefs, Pix *pixels) {
    const int b = (int)(unit - K.unit0) * HVC_MIXED_UNIT + lane, nblk = K.nblk;
    const bool active = b < nblk;
    MixedBlock<N, Coef, Pix> r = mixed_block_at<N>(K, active ? b : nblk - 1, coefs, pixels);
    r.active = active;
    return r;
}

// the 128-byte record as eight 16-byte loads
__device__ __forceinline__ void mixed_load_record(const int16_t *rec, unsigned (&w)[32]) {
    const uint4 *src = reinterpret_cast<const uint4 *>(rec);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint4 t = src[j];
        w[4 * j + 0] = t.x;
        w[4 * j + 1] = t.y;
        w[4 * j + 2] = t.z;
        w[4 * j + 3] = t.w;
    }
}

// ---------------------------------------------------------------------------
// The lane of an image: any descriptor with unit0, lanes, groups, magic.  Both forms return whether the lane exists and
// fill r only if it does.
struct MixedImageLane {
    unsigned t;          // lane inside the image (mixed_image_row_lane: inside the row)
    unsigned row, group; // t / groups, t % groups (mixed_image_row_lane: of the unit; wave-uniform)
};
template <class ImageK>
__device__ __forceinline__ bool mixed_image_lane(const ImageK &K, unsigned unit, int lane, MixedImageLane &r) {
    r.t = (unit - K.unit0) * HVC_MIXED_UNIT + (unsigned)lane;
    if (r.t >= K.lanes) return false;
    r.row = K.groups == 1 ? r.t : __umulhi(r.t, K.magic);
    r.group = r.t - r.row * K.groups;
    return true;
}
// a unit = 64 consecutive lanes of ONE ROW: the unit is split into (row, unit of the row), K.lanes counts a row's lanes
template <class ImageK>
__device__ __forceinline__ bool mixed_image_row_lane(const ImageK &K, unsigned unit, int lane, MixedImageLane &r) {
    const unsigned u = unit - K.unit0;
    r.row = K.groups == 1 ? u : __umulhi(u, K.magic);
    r.group = u - r.row * K.groups;
    r.t = r.group * HVC_MIXED_UNIT + (unsigned)lane;
    return r.t < K.lanes;
}

// the image as the single-geometry colour kernels' parameter block: one frame, its own bases
__device__ __forceinline__ RgbOp mixed_rgb_op(const MixedRgbParams &P, const MixedRgbImageK &K) {
    RgbOp R;
    R.y = const_cast<uint8_t *>(P.yuv) + K.y_base;
    R.cb = const_cast<uint8_t *>(P.yuv) + K.cb_base;
    R.cr = const_cast<uint8_t *>(P.yuv) + K.cr_base;
    R.rgb = P.rgb + K.rgb_base;
    R.y_stride = K.y_stride, R.cb_stride = K.cb_stride, R.cr_stride = K.cr_stride, R.yuv_fs = 0;
    R.row_stride = K.row_stride, R.plane_stride = K.plane_stride, R.frame_stride = 0;
    R.w = K.w, R.h = K.h, R.cw = K.cw, R.ch = K.ch;
    R.vec_y = K.vec_y, R.vec_c = K.vec_c, R.vec_rgb = K.vec_rgb;
    return R;
}
// The wave-uniform branch on the sampling.  Lane: a struct with `template <int S, int PLANAR> static void lane(const RgbOp &,
// unsigned row, unsigned group)`.
template <class Lane, int PLANAR>
__device__ __forceinline__ void mixed_rgb_dispatch(int sampling, const RgbOp &R, unsigned row, unsigned group) {
    switch (sampling) {
    case HVC_YUV_420: Lane::template lane<420, PLANAR>(R, row, group); break;
    case HVC_YUV_422: Lane::template lane<422, PLANAR>(R, row, group); break;
    case HVC_YUV_444: Lane::template lane<444, PLANAR>(R, row, group); break;
    default: Lane::template lane<400, PLANAR>(R, row, group); break;
    }
}

// ---------------------------------------------------------------------------
// The host launcher: one launch of `kernel` over all units of P, HVC_MIXED_GROUP units per workgroup; k0 / k1 (optional)
// bracket it; n_units == 0 launches nothing.  extra: the kernel's arguments after its parameter block.
inline unsigned mixed_groups(unsigned n_units) { return (n_units + HVC_MIXED_GROUP - 1) / HVC_MIXED_GROUP; }

template <class Params, class... KArgs, class... Args>
inline hipError_t mixed_launch(void (*kernel)(Params, KArgs...), const Params &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1,
                               Args... extra) {
    if (P.n_units == 0) return hipSuccess;
    hipError_t e;
    if (k0 && (e = hipEventRecord(k0, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(mixed_groups(P.n_units)), dim3(HVC_MIXED_LANES), 0, s, P, extra...);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (k1 && (e = hipEventRecord(k1, s)) != hipSuccess) return e;
    return hipSuccess;
}
// the kernels that take their groups through mixed_wave_xcd: the map for this grid on a copy of the block
template <class Params>
inline hipError_t mixed_launch_xcd(void (*kernel)(Params), const Params &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    Params Q = P;
    Q.xcd_map = xcd_map_for(mixed_groups(P.n_units), 1, Q.xcd_magic); // (0 beyond 65535 groups: the plain order)
    return mixed_launch(kernel, Q, s, k0, k1);
}

} // namespace
} // namespace hvc
#endif
