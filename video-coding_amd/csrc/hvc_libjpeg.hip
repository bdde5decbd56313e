// hvc_libjpeg.hip -- the two kernels of hvc_set_arithmetic(HVC_ARITH_LIBJPEG): the decoder of include/hvc_jpeg.h
// ("Bit-exact to libjpeg"; numpy restatement: tools/libjpeg_reference.py).
//
// k_islow: coefficient records -> planes by libjpeg's jidctint.c inverse DCT.  Mapping: k_hardcaml's / k_decode_packed's --
// one 8x8 block per lane, a tile of HVC_TILE consecutive blocks of one plane per workgroup, grid = tiles x frames,
// workgroups -> (frame, tile) by xcd_work.  A lane loads its 128-byte record (8 x 16 B), keeps all 64 values in VGPRs and
// stores 8 rows of 8 bytes: the kernel moves the model path's bytes.  No LDS, no scratch.
//   guard       S = SUM |coefficient| * table entry, exact and saturating: v_pk_sub_i16 + v_pk_max_i16 for the magnitudes,
//               v_dot2_u32_u16 with clamp against the table pair of each record dword (hvc_islow_spec.h)
//   int path    (S <= HVC_IS_GUARD_SUM) dequantisation by v_pk_mul_lo_u16 per record dword -- every product fits int16 --,
//               the step of hvc_islow_spec.h on int with v_mul_i32_i24 products in both passes (tests/test_islow_guard.py
//               proves the bounds); pass 2's rounding and the level shift ride in one addend, shift and saturation by
//               v_ashr_pk_u8_i32
//   int64 path  every other block, in the same lane (a rare divergent branch): the same step as its 8 x 8 integer matrix
//               (made from the list at compile time) on long long, in real loops over a record read again from the cache,
//               so that the path needs no registers beyond the int path's; counted in P.wide_total with one atomic per
//               wavefront that has such a block
// Both paths give the definition's value for every int16 coefficient and every 16-bit table entry.
//
// k_ycc_to_rgb_fancy: k_ycc_to_rgb's lane (hvc_rgb.hip: 8 columns of one row, of two rows for 4:2:0) with libjpeg's
// "fancy" triangle filter in place of the model's supersampling; loads of Y, colour matrix and stores are the shared
// code of hvc_rgb_dev.h (8-byte and byte-wise paths, interleaved and planar, strides).  A lane reads its four chroma
// samples of a row as one dword where alignment allows and its two neighbours, clamped to the chroma WINDOW, as byte LOADS
// (not DPP: the neighbours of a wavefront's end lanes and of a lane row's ends would need the loads anyway, and the bytes
// sit in lines the adjacent lanes have just fetched); 4:2:0 reads three window rows.  The clamp gives libjpeg's edge
// rules by itself: (3 s + s + 1) >> 2 = s, (3 t + t + 8) >> 4 = (4 t + 8) >> 4.  Windows at most 2 samples wide are replicated
// (libjpeg picks its plain routine there): an image-uniform branch.
//
// The block code (hvc_islow_dev.h) and the colour pass's lane (hvc_fancy_dev.h) are device headers: the kernels over mixed
// batches, k_islow_mixed and k_ycc_to_rgb_fancy_mixed (hvc_mixed_libjpeg.hip), expand the same code.
#include "hvc_ctx.h"
#include "hvc_fancy_dev.h"
#include "hvc_islow_dev.h"
#include "hvc_libjpeg.h"

namespace hvc {
namespace {

// DCP: the DC comes from P.dc_plane
template <bool DCP>
__global__ __launch_bounds__(HVC_TILE) void k_islow(IslowParams P) {
    const int lane = threadIdx.x;
    unsigned wframe, wtile;
    xcd_work(P.xcd_map, P.xcd_magic, wframe, wtile);
    int c = 0;
#pragma unroll
    for (int i = 1; i < HVC_MAX_COMP; i++)
        if (i < P.n_comp && (int)wtile >= P.comp[i].tile0) c = i;
    const CompK &K = P.comp[c];
    int b = ((int)wtile - K.tile0) * HVC_TILE + lane;
    const bool active = b < K.nblk;
    b = active ? b : K.nblk - 1; // (inactive lanes compute the plane's last block and store nothing)
    const unsigned by = K.bw == 1 ? (unsigned)b : __umulhi((unsigned)b, K.magic);
    const unsigned bx = (unsigned)b - by * (unsigned)K.bw;
    const size_t coef_idx = (size_t)wframe * P.coef_fs + K.coef_off + (size_t)b * 64;
    uint8_t *dst = P.pixels + (size_t)wframe * P.pixel_fs + K.plane_off + (size_t)by * 8 * K.stride + (size_t)bx * 8;
    const unsigned *__restrict__ qq = P.qq + K.qtab * 32; // wave-uniform, kernarg segment

    unsigned w[32];
    const uint4 *src = reinterpret_cast<const uint4 *>(P.coefs + coef_idx);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint4 t = src[j];
        w[4 * j + 0] = t.x;
        w[4 * j + 1] = t.y;
        w[4 * j + 2] = t.z;
        w[4 * j + 3] = t.w;
    }
    if (DCP) w[0] = (w[0] & 0xffff0000u) | (unsigned)(unsigned short)P.dc_plane[(size_t)wframe * P.dc_fs + (K.coef_off >> 6) + (size_t)b];

    const unsigned sum = islow_guard_sum(w, qq);
    const bool narrow = !P.all_wide && sum <= (unsigned)HVC_IS_GUARD_SUM;
    if (narrow) {
        unsigned out[8][2];
        islow_block_int(w, qq, out);
        if (active) {
#pragma unroll
            for (int j = 0; j < 8; j++) store_row8_nt(dst + (size_t)j * K.stride, out[j][0], out[j][1]);
        }
    } else {
        islow_block_wide(P.coefs + coef_idx, half_of(w, 0), qq, dst, K.stride, active);
    }
    if (!P.all_wide) {
        const unsigned long long m = __ballot(active && !narrow);
        if (m && (lane & 63) == 0) atomicAdd(P.wide_total, (unsigned long long)__popcll(m));
    }
}

} // namespace

void prepare_islow_tables(const uint16_t *qtabs, int n_qtabs, unsigned *qq) {
    for (int t = 0; t < n_qtabs; t++)
        for (int i = 0; i < 32; i++) qq[t * 32 + i] = (unsigned)qtabs[t * 64 + 2 * i] | (unsigned)qtabs[t * 64 + 2 * i + 1] << 16;
}

hipError_t launch_islow(const IslowParams &P, hipStream_t s, hipEvent_t k0, hipEvent_t k1) {
    if (P.n_frames <= 0 || P.tiles_per_frame <= 0) return hipSuccess;
    hipError_t e;
    const dim3 grid((unsigned)P.tiles_per_frame, (unsigned)P.n_frames, 1);
    IslowParams Q = P;
    Q.xcd_map = xcd_map_for(grid.x, grid.y, Q.xcd_magic);
    if (k0 && (e = hipEventRecord(k0, s)) != hipSuccess) return e;
    if (P.dc_plane) hipLaunchKernelGGL(k_islow<true>, grid, dim3(HVC_TILE), 0, s, Q);
    else hipLaunchKernelGGL(k_islow<false>, grid, dim3(HVC_TILE), 0, s, Q);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (k1 && (e = hipEventRecord(k1, s)) != hipSuccess) return e;
    return hipSuccess;
}

} // namespace hvc

// ---------------------------------------------------------------------------
// The colour pass with libjpeg's fancy upsampling
namespace {

// S: 420, 422, 444 or 400 (luma only).  Lanes: ceil(w / 8) per lane row; a lane row is one image row (4:2:0: two).
template <int S, int PLANAR>
__global__ __launch_bounds__(256) void k_ycc_to_rgb_fancy(RgbOp P) {
    const unsigned groups = (unsigned)(P.w + 7) >> 3, lrows = S == 420 ? (unsigned)(P.h + 1) >> 1 : (unsigned)P.h;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups * lrows) return;
    const unsigned lr = t / groups, g = t - lr * groups;
    const size_t f = blockIdx.y;
    HVC_YCC_LANE_TO_RGB_FANCY(P, f, lr, g);
}

template <int PLANAR>
void launch_fancy(int sampling, dim3 grid, hipStream_t s, const RgbOp &P) {
    switch (sampling) {
    case HVC_YUV_420: hipLaunchKernelGGL((k_ycc_to_rgb_fancy<420, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_422: hipLaunchKernelGGL((k_ycc_to_rgb_fancy<422, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_444: hipLaunchKernelGGL((k_ycc_to_rgb_fancy<444, PLANAR>), grid, dim3(256), 0, s, P); break;
    default: hipLaunchKernelGGL((k_ycc_to_rgb_fancy<400, PLANAR>), grid, dim3(256), 0, s, P); break;
    }
}

} // namespace

// ycc_to_rgb_device (hvc_rgb.hip) with k_ycc_to_rgb_fancy: the same arguments, the same launches of at most 65535 frames
hipError_t ycc_to_rgb_fancy_device(const uint8_t *d_yuv, size_t yuv_fs, const hvc_component *comps, int sampling, int w, int h, int cw,
                                   int ch, int n_frames, uint8_t *d_rgb, const RgbImage &im, hipStream_t s) {
    if (n_frames <= 0 || w <= 0 || h <= 0) return hipSuccess;
    const bool grey = sampling == HVC_YUV_400;
    RgbOp P;
    std::memset(&P, 0, sizeof P);
    P.w = w, P.h = h, P.cw = cw, P.ch = ch;
    P.y_stride = comps[0].stride;
    P.cb_stride = grey ? 0 : comps[1].stride, P.cr_stride = grey ? 0 : comps[2].stride;
    P.yuv_fs = yuv_fs;
    P.row_stride = im.row_stride, P.frame_stride = im.frame_stride, P.plane_stride = im.row_stride * (size_t)h;
    const unsigned lrows = sampling == HVC_YUV_420 ? (unsigned)(h + 1) >> 1 : (unsigned)h;
    const unsigned long long lanes = (unsigned long long)((w + 7) >> 3) * lrows;
    for (int f0 = 0; f0 < n_frames; f0 += 65535) {
        const int cnt = n_frames - f0 < 65535 ? n_frames - f0 : 65535;
        uint8_t *base = const_cast<uint8_t *>(d_yuv) + (size_t)f0 * yuv_fs;
        P.y = base + comps[0].plane_offset;
        P.cb = grey ? nullptr : base + comps[1].plane_offset;
        P.cr = grey ? nullptr : base + comps[2].plane_offset;
        P.rgb = d_rgb + (size_t)f0 * im.frame_stride;
        const size_t ca = sampling == HVC_YUV_444 ? 8 : 4;
        P.vec_y = ((uintptr_t)P.y | P.y_stride | yuv_fs) % 8 == 0;
        P.vec_c = !grey && ((uintptr_t)P.cb | (uintptr_t)P.cr | P.cb_stride | P.cr_stride | yuv_fs) % ca == 0;
        P.vec_rgb = ((uintptr_t)P.rgb | P.row_stride | P.frame_stride | (im.layout == HVC_RGB_PLANAR ? P.plane_stride : 0)) % 8 == 0;
        const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)cnt, 1);
        if (im.layout == HVC_RGB_PLANAR) launch_fancy<1>(sampling, grid, s, P);
        else launch_fancy<0>(sampling, grid, s, P);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
