// hvc_mixed_libjpeg.hip -- the two kernels of hvc_set_mixed_arithmetic(HVC_ARITH_LIBJPEG): the decoder of include/hvc_jpeg.h
// ("Bit-exact to libjpeg") over frames and images of DIFFERENT geometry, sampling and quantiser tables in one launch.
//
// k_islow_mixed: k_islow's block (hvc_islow_dev.h: guard sum, int path, int64 path in the same lane -- the same expansion of
// hvc_islow_spec.h, no second spelling) under the block stage's decomposition of hvc_mixed_dev.h.  No LDS, no scratch.
//   table       32 dwords q[2i] | q[2i+1] << 16 per distinct table of the plan (mixed_islow_pairs_build: IslowParams::qq's form,
//               all 16 bits of every entry), beside the plan image; read through a wave-uniform const pointer, so that the
//               words arrive in SGPRs, where k_islow finds its kernarg copy
//   wide path   a block outside HVC_IS_GUARD_SUM takes the int64 path in its own lane: no fix-up list, no per-table flag;
//               counted in P.wide_total with one atomic per wavefront that has such a block
//   DC          the record's coefficient 0: the mixed pipelines keep absolute DCs in the records
//
// k_ycc_to_rgb_fancy_mixed: k_ycc_to_rgb_fancy's lane (HVC_YCC_LANE_TO_RGB_FANCY, hvc_fancy_dev.h) in k_ycc_to_rgb_mixed's frame
// (hvc_mixed_rgb.hip; the image passes of hvc_mixed_dev.h).  The descriptor's cw x ch is the chroma window the triangle
// filter clamps to.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hvc_jpeg.h"
#include "hvc_fancy_dev.h"
#include "hvc_islow_dev.h"
#include "hvc_mixed_dev.h"
#include "hvc_mixed_libjpeg.h"

namespace hvc {
namespace {

static_assert(HVC_ISLOW_PAIR_WORDS == 32, "a lane's table: one pair word per record dword");

__global__ __launch_bounds__(HVC_MIXED_LANES) void k_islow_mixed(MixedIslowParams P) {
    unsigned wf, wt;
    xcd_work(P.xcd_map, P.xcd_magic, wf, wt); // gridDim.y == 1: a permutation of the groups (or the plain order)
    const unsigned group = wf * gridDim.x + wt;
    const int lane = threadIdx.x & (HVC_MIXED_UNIT - 1);
    const unsigned unit = (unsigned)__builtin_amdgcn_readfirstlane((int)(group * HVC_MIXED_GROUP + (threadIdx.x >> 6)));
    if (unit >= P.n_units) return; // (the whole wavefront: the last group's spare units)
    const MixedPlaneK &K = P.planes[P.map[unit]];
    const unsigned *__restrict__ qq = P.pairs + (size_t)K.table * HVC_ISLOW_PAIR_WORDS; // wave-uniform
    int b = (int)(unit - K.unit0) * HVC_MIXED_UNIT + lane;
    const bool active = b < K.nblk;
    b = active ? b : K.nblk - 1; // (inactive lanes compute the plane's last block and store nothing)
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const unsigned bx = (unsigned)b - by * (unsigned)K.bw;
    const size_t stride = (size_t)K.stride;
    const int16_t *rec = P.coefs + (size_t)K.coef_base + (size_t)b * 64;
    uint8_t *dst = P.pixels + (size_t)K.pix_base + (size_t)by * 8 * stride + (size_t)bx * 8;

    unsigned w[32];
    const uint4 *src = reinterpret_cast<const uint4 *>(rec);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint4 t = src[j];
        w[4 * j + 0] = t.x;
        w[4 * j + 1] = t.y;
        w[4 * j + 2] = t.z;
        w[4 * j + 3] = t.w;
    }

    const unsigned sum = islow_guard_sum(w, qq);
    const bool narrow = !P.all_wide && sum <= (unsigned)HVC_IS_GUARD_SUM;
    if (narrow) {
        unsigned out[8][2];
        islow_block_int(w, qq, out);
        if (active) {
#pragma unroll
            for (int j = 0; j < 8; j++) store_row8_nt(dst + (size_t)j * stride, out[j][0], out[j][1]);
        }
    } else {
        islow_block_wide(rec, half_of(w, 0), qq, dst, stride, active);
    }
    if (!P.all_wide) {
        const unsigned long long m = __ballot(active && !narrow);
        if (m && lane == 0) atomicAdd(P.wide_total, (unsigned long long)__popcll(m));
    }
}

struct FancyLane {
    template <int S, int PLANAR>
    static __device__ __forceinline__ void lane(const RgbOp &P, unsigned lr, unsigned g) {
        const size_t f = 0; // one image per RgbOp
        HVC_YCC_LANE_TO_RGB_FANCY(P, f, lr, g);
    }
};

template <int PLANAR>
__global__ __launch_bounds__(HVC_MIXED_LANES) void k_ycc_to_rgb_fancy_mixed(MixedRgbParams P) {
    const MixedWave W = mixed_wave_plain();
    if (W.unit >= P.n_units) return;
    const MixedRgbImageK K = P.images[P.map[W.unit]]; // wave-uniform: read once, before any store
    MixedImageLane L;
    if (!mixed_image_lane(K, W.unit, W.lane, L)) return;
    mixed_rgb_dispatch<FancyLane, PLANAR>(K.sampling, mixed_rgb_op(P, K), L.row, L.group);
}

} // namespace

hipError_t launch_islow_mixed(const MixedIslowParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    return mixed_launch_xcd(k_islow_mixed, P, s, k0, k1);
}

hipError_t launch_ycc_to_rgb_fancy_mixed(const MixedRgbParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    return mixed_launch(P.planar ? k_ycc_to_rgb_fancy_mixed<1> : k_ycc_to_rgb_fancy_mixed<0>, P, s, k0, k1);
}

} // namespace hvc
