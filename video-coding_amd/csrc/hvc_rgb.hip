// hvc_rgb.hip -- JFIF colour conversion (ITU-T T.871) in both directions, fused with the chroma resampling in front of /
// behind it: decoded planes -> RGB (k_ycc_to_rgb) and RGB -> the encoder's planes (k_rgb_to_ycc).  The definition every
// byte is tested against (tools/rgb_reference.py):
//     full-size chroma   Planar_444.supersample_hv2 (4:2:0) / supersample_h2 (4:2:2) of the cw x ch window of the chroma
//                        planes (tools/src/planar_444.ml:25-33, 82-103: avg2 / avg4, last column and row repeated)
//     colour             libjpeg's 16-bit fixed-point form of the JFIF matrix, cb = Cb - 128, cr = Cr - 128, >> arithmetic:
//                          R = clamp(Y + ((  91881 cr              + 32768) >> 16))
//                          G = clamp(Y + (( -22554 cb - 46802 cr   + 32768) >> 16))
//                          B = clamp(Y + (( 116130 cb              + 32768) >> 16))
//                        and back (every output is in 0 .. 255 already):
//                          Y  = ( 19595 R + 38470 G +  7471 B               + 32768) >> 16
//                          Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//                          Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
//     sub-sampling       Planar_444.subsample_hv2 / subsample_h2 (planar_444.ml:18-23, 69-80)
// Three components are always Y, Cb, Cr (no Adobe APP14 transform flag, no CMYK).  Both kernels are byte traffic: a lane
// owns 8 columns of one row (4:2:0: of two rows, so that a chroma row is loaded once for both); the full-size chroma planes
// exist in registers only.  Rows whose bases and strides allow it move as 8-byte pieces, everything else through the
// bounds-checked byte path.  The entry points live with their families: hvc_yuv_to_rgb / hvc_rgb_to_yuv in hvc_yuv.hip,
// hvc_decode_frames_rgb in hvc_capi.hip, the file-level ones in hvc_capi_jpeg.hip.
#include "hvc_ctx.h"

namespace {

struct RgbOp {
    uint8_t *y, *cb, *cr; // frame 0's planes (source: k_ycc_to_rgb, destination: k_rgb_to_ycc)
    uint8_t *rgb;
    size_t y_stride, cb_stride, cr_stride, yuv_fs; // bytes per row of each plane, from frame to frame
    size_t row_stride, plane_stride, frame_stride; // of the RGB image (plane_stride: planar layout)
    int w, h, cw, ch;                              // frame size; valid chroma samples (k_ycc_to_rgb: where the neighbours clamp)
    int vec_y, vec_c, vec_rgb;                     // bases and strides allow the 8 / 4-byte forms
};

typedef unsigned u2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned avg2x4(unsigned a, unsigned b) { // (a + b + 1) >> 1 on four bytes (planar_444.ml:4-8)
    return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu);
}
// avg4 on four samples at once (tests/test_guard_bounds.py::test_avg4_by_lerp_identity, as in hvc_yuv.hip)
__device__ __forceinline__ unsigned avg4x4(unsigned a, unsigned b, unsigned c, unsigned d) {
    return __builtin_amdgcn_lerp(__builtin_amdgcn_lerp(a, b, 0x01010101u), __builtin_amdgcn_lerp(c, d, 0u), ~(a ^ b) | (c ^ d));
}
__device__ __forceinline__ unsigned pairsum(unsigned x) { return (x & 0x00ff00ffu) + ((x >> 8) & 0x00ff00ffu); }
__device__ __forceinline__ unsigned pack_even(unsigned lo, unsigned hi) { // bytes 0 and 2 of lo, then of hi
    return __builtin_amdgcn_perm(hi, lo, 0x06040200u);
}

// samples x0 .. x0 + 7 of a row of n valid samples (columns past the last one repeat it: never read, or never used)
__device__ __forceinline__ void load8(const uint8_t *row, int x0, int n, bool vec, unsigned &lo, unsigned &hi) {
    if (vec) {
        const u2v v = __builtin_nontemporal_load(reinterpret_cast<const u2v *>(row + x0));
        lo = v.x, hi = v.y;
        return;
    }
    lo = hi = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        lo |= (unsigned)row[min(x0 + i, n - 1)] << (8 * i);
        hi |= (unsigned)row[min(x0 + 4 + i, n - 1)] << (8 * i);
    }
}
// samples c0 .. c0 + 3 of a chroma row of n valid samples and every one's right neighbour (the last column's: itself)
__device__ __forceinline__ void load4n(const uint8_t *row, int c0, int n, bool vec, unsigned &a, unsigned &nb) {
    if (vec) {
        a = *reinterpret_cast<const unsigned *>(row + c0);
    } else {
        a = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) a |= (unsigned)row[min(c0 + i, n - 1)] << (8 * i);
    }
    nb = (a >> 8) | ((unsigned)row[min(c0 + 4, n - 1)] << 24);
}
// (e0 o0 e1 o1) (e2 o2 e3 o3): the even and odd columns of a supersampled row, side by side
__device__ __forceinline__ void interleave(unsigned even, unsigned odd, unsigned &lo, unsigned &hi) {
    lo = __builtin_amdgcn_perm(odd, even, 0x05010400u);
    hi = __builtin_amdgcn_perm(odd, even, 0x07030602u);
}
__device__ __forceinline__ void store8(uint8_t *row, int x0, int n, bool vec, unsigned lo, unsigned hi) {
    if (vec) {
        const u2v v = {lo, hi};
        __builtin_nontemporal_store(v, reinterpret_cast<u2v *>(row + x0));
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (x0 + i < n) row[x0 + i] = (uint8_t)((i < 4 ? lo >> (8 * i) : hi >> (8 * (i - 4))) & 0xffu);
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// four pixels: packed Y, Cb, Cr -> packed R, G, B
__device__ __forceinline__ void ycc4_to_rgb(unsigned y, unsigned cb, unsigned cr, unsigned &r, unsigned &g, unsigned &b) {
    r = g = b = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int Y = (int)((y >> (8 * i)) & 0xffu), u = (int)((cb >> (8 * i)) & 0xffu) - 128, v = (int)((cr >> (8 * i)) & 0xffu) - 128;
        r |= (unsigned)clamp255(Y + ((91881 * v + 32768) >> 16)) << (8 * i);
        g |= (unsigned)clamp255(Y + ((-22554 * u - 46802 * v + 32768) >> 16)) << (8 * i);
        b |= (unsigned)clamp255(Y + ((116130 * u + 32768) >> 16)) << (8 * i);
    }
}
__device__ __forceinline__ void rgb4_to_ycc(unsigned r, unsigned g, unsigned b, unsigned &y, unsigned &cb, unsigned &cr) {
    y = cb = cr = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int R = (int)((r >> (8 * i)) & 0xffu), G = (int)((g >> (8 * i)) & 0xffu), B = (int)((b >> (8 * i)) & 0xffu);
        y |= (unsigned)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) << (8 * i);
        cb |= (unsigned)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16) << (8 * i);
        cr |= (unsigned)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16) << (8 * i);
    }
}

// four pixels R G B R | G B R G | B R G B <-> packed R, G, B (v_perm_b32: selector bytes 0 .. 3 = the second operand)
__device__ __forceinline__ void rgb_interleave(unsigned r, unsigned g, unsigned b, unsigned &d0, unsigned &d1, unsigned &d2) {
    d0 = __builtin_amdgcn_perm(b, __builtin_amdgcn_perm(g, r, 0x01000400u), 0x03040100u);
    d1 = __builtin_amdgcn_perm(b, __builtin_amdgcn_perm(g, r, 0x06020005u), 0x03020500u);
    d2 = __builtin_amdgcn_perm(b, __builtin_amdgcn_perm(g, r, 0x00070300u), 0x07020106u);
}
__device__ __forceinline__ void rgb_deinterleave(unsigned d0, unsigned d1, unsigned d2, unsigned &r, unsigned &g, unsigned &b) {
    r = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00060300u), 0x05020100u);
    g = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00070401u), 0x06020100u);
    b = __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, 0x00000502u), 0x07040100u);
}

// columns x0 .. x0 + 7 of one RGB row
template <int PLANAR>
__device__ __forceinline__ void store_rgb(const RgbOp &P, uint8_t *frame, int row, int x0, bool vec, const unsigned r[2], const unsigned g[2],
                                          const unsigned b[2]) {
    uint8_t *line = frame + (size_t)row * P.row_stride;
    if (PLANAR) {
        store8(line, x0, P.w, vec, r[0], r[1]);
        store8(line + P.plane_stride, x0, P.w, vec, g[0], g[1]);
        store8(line + 2 * P.plane_stride, x0, P.w, vec, b[0], b[1]);
        return;
    }
    if (vec) {
        unsigned d[6];
        rgb_interleave(r[0], g[0], b[0], d[0], d[1], d[2]);
        rgb_interleave(r[1], g[1], b[1], d[3], d[4], d[5]);
        u2v *o = reinterpret_cast<u2v *>(line + 3 * (size_t)x0);
        const u2v o0 = {d[0], d[1]}, o1 = {d[2], d[3]}, o2 = {d[4], d[5]};
        __builtin_nontemporal_store(o0, o);
        __builtin_nontemporal_store(o1, o + 1);
        __builtin_nontemporal_store(o2, o + 2);
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (x0 + i < P.w) {
            uint8_t *px = line + 3 * (size_t)(x0 + i);
            px[0] = (uint8_t)((r[i >> 2] >> (8 * (i & 3))) & 0xffu);
            px[1] = (uint8_t)((g[i >> 2] >> (8 * (i & 3))) & 0xffu);
            px[2] = (uint8_t)((b[i >> 2] >> (8 * (i & 3))) & 0xffu);
        }
}
template <int PLANAR>
__device__ __forceinline__ void load_rgb(const RgbOp &P, const uint8_t *frame, int row, int x0, bool vec, unsigned r[2], unsigned g[2], unsigned b[2]) {
    const uint8_t *line = frame + (size_t)row * P.row_stride;
    if (PLANAR) {
        load8(line, x0, P.w, vec, r[0], r[1]);
        load8(line + P.plane_stride, x0, P.w, vec, g[0], g[1]);
        load8(line + 2 * P.plane_stride, x0, P.w, vec, b[0], b[1]);
        return;
    }
    if (vec) {
        const u2v *s = reinterpret_cast<const u2v *>(line + 3 * (size_t)x0);
        const u2v a0 = __builtin_nontemporal_load(s), a1 = __builtin_nontemporal_load(s + 1), a2 = __builtin_nontemporal_load(s + 2);
        rgb_deinterleave(a0.x, a0.y, a1.x, r[0], g[0], b[0]);
        rgb_deinterleave(a1.y, a2.x, a2.y, r[1], g[1], b[1]);
        return;
    }
    r[0] = r[1] = g[0] = g[1] = b[0] = b[1] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t *px = line + 3 * (size_t)min(x0 + i, P.w - 1);
        r[i >> 2] |= (unsigned)px[0] << (8 * (i & 3));
        g[i >> 2] |= (unsigned)px[1] << (8 * (i & 3));
        b[i >> 2] |= (unsigned)px[2] << (8 * (i & 3));
    }
}

// S: 420, 422, 444 or 400 (luma only).  Lanes: ceil(w / 8) per lane row; a lane row is one image row (4:2:0: two).
template <int S, int PLANAR>
__global__ __launch_bounds__(256) void k_ycc_to_rgb(RgbOp P) {
    constexpr int ROWS = S == 420 ? 2 : 1;
    const unsigned groups = (unsigned)(P.w + 7) >> 3, lrows = S == 420 ? (unsigned)(P.h + 1) >> 1 : (unsigned)P.h;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups * lrows) return;
    const unsigned lr = t / groups, g = t - lr * groups;
    const size_t f = blockIdx.y;
    const int x0 = (int)(8 * g);
    const bool full = x0 + 8 <= P.w;
    unsigned cb[ROWS][2], cr[ROWS][2];
    if (S == 444) {
        load8(P.cb + f * P.yuv_fs + (size_t)lr * P.cb_stride, x0, P.cw, P.vec_c && full, cb[0][0], cb[0][1]);
        load8(P.cr + f * P.yuv_fs + (size_t)lr * P.cr_stride, x0, P.cw, P.vec_c && full, cr[0][0], cr[0][1]);
    } else if (S != 400) {
        const int c0 = (int)(4 * g);
        const bool vc = P.vec_c && c0 + 4 <= P.cw;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const uint8_t *plane = (k ? P.cr : P.cb) + f * P.yuv_fs;
            const size_t stride = k ? P.cr_stride : P.cb_stride;
            unsigned(*out)[2] = k ? cr : cb;
            unsigned a, an;
            load4n(plane + (size_t)lr * stride, c0, P.cw, vc, a, an);
            interleave(a, avg2x4(a, an), out[0][0], out[0][1]); // dst[2c] = a, dst[2c + 1] = avg2 a b
            if (S == 420) { // the row below: avg2 a c, avg4 a b c d; the last chroma row: itself
                unsigned c, cn;
                load4n(plane + (size_t)min(lr + 1u, (unsigned)P.ch - 1u) * stride, c0, P.cw, vc, c, cn);
                interleave(avg2x4(a, c), avg4x4(a, an, c, cn), out[ROWS - 1][0], out[ROWS - 1][1]);
            }
        }
    }
    uint8_t *frame = P.rgb + f * P.frame_stride;
#pragma unroll
    for (int rr = 0; rr < ROWS; rr++) {
        const int row = (int)lr * ROWS + rr;
        if (row >= P.h) break;
        unsigned y[2], r[2], gg[2], b[2];
        load8(P.y + f * P.yuv_fs + (size_t)row * P.y_stride, x0, P.w, P.vec_y && full, y[0], y[1]);
        if (S == 400) {
            r[0] = gg[0] = b[0] = y[0];
            r[1] = gg[1] = b[1] = y[1];
        } else {
            ycc4_to_rgb(y[0], cb[rr][0], cr[rr][0], r[0], gg[0], b[0]);
            ycc4_to_rgb(y[1], cb[rr][1], cr[rr][1], r[1], gg[1], b[1]);
        }
        store_rgb<PLANAR>(P, frame, row, x0, P.vec_rgb && full, r, gg, b);
    }
}

// The way back; w even for 4:2:2 and 4:2:0, h even for 4:2:0 (the launch checks).  A lane's 8 columns give 4 chroma samples.
template <int S, int PLANAR>
__global__ __launch_bounds__(256) void k_rgb_to_ycc(RgbOp P) {
    constexpr int ROWS = S == 420 ? 2 : 1;
    const unsigned groups = (unsigned)(P.w + 7) >> 3, lrows = S == 420 ? (unsigned)P.h >> 1 : (unsigned)P.h;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups * lrows) return;
    const unsigned lr = t / groups, g = t - lr * groups;
    const size_t f = blockIdx.y;
    const int x0 = (int)(8 * g);
    const bool full = x0 + 8 <= P.w;
    const uint8_t *frame = P.rgb + f * P.frame_stride;
    unsigned cb[ROWS][2], cr[ROWS][2];
#pragma unroll
    for (int rr = 0; rr < ROWS; rr++) {
        const int row = (int)lr * ROWS + rr;
        unsigned r[2], gg[2], b[2], y[2];
        load_rgb<PLANAR>(P, frame, row, x0, P.vec_rgb && full, r, gg, b);
        rgb4_to_ycc(r[0], gg[0], b[0], y[0], cb[rr][0], cr[rr][0]);
        rgb4_to_ycc(r[1], gg[1], b[1], y[1], cb[rr][1], cr[rr][1]);
        store8(P.y + f * P.yuv_fs + (size_t)row * P.y_stride, x0, P.w, P.vec_y && full, y[0], y[1]);
    }
    if (S == 400) return;
    uint8_t *pcb = P.cb + f * P.yuv_fs + (size_t)lr * P.cb_stride, *pcr = P.cr + f * P.yuv_fs + (size_t)lr * P.cr_stride;
    if (S == 444) {
        store8(pcb, x0, P.w, P.vec_c && full, cb[0][0], cb[0][1]);
        store8(pcr, x0, P.w, P.vec_c && full, cr[0][0], cr[0][1]);
        return;
    }
    unsigned ob, orr;
    if (S == 422) { // subsample_h2: avg2 of the pair
        ob = pack_even(((pairsum(cb[0][0]) + 0x00010001u) >> 1) & 0x00ff00ffu, ((pairsum(cb[0][1]) + 0x00010001u) >> 1) & 0x00ff00ffu);
        orr = pack_even(((pairsum(cr[0][0]) + 0x00010001u) >> 1) & 0x00ff00ffu, ((pairsum(cr[0][1]) + 0x00010001u) >> 1) & 0x00ff00ffu);
    } else { // subsample_hv2: avg4 of the 2 x 2
        ob = pack_even(((pairsum(cb[0][0]) + pairsum(cb[ROWS - 1][0]) + 0x00020002u) >> 2) & 0x00ff00ffu,
                       ((pairsum(cb[0][1]) + pairsum(cb[ROWS - 1][1]) + 0x00020002u) >> 2) & 0x00ff00ffu);
        orr = pack_even(((pairsum(cr[0][0]) + pairsum(cr[ROWS - 1][0]) + 0x00020002u) >> 2) & 0x00ff00ffu,
                        ((pairsum(cr[0][1]) + pairsum(cr[ROWS - 1][1]) + 0x00020002u) >> 2) & 0x00ff00ffu);
    }
    const int c0 = (int)(4 * g), cw = P.w >> 1;
    if (P.vec_c && full) {
        __builtin_nontemporal_store(ob, reinterpret_cast<unsigned *>(pcb + c0));
        __builtin_nontemporal_store(orr, reinterpret_cast<unsigned *>(pcr + c0));
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (c0 + i < cw) {
            pcb[c0 + i] = (uint8_t)((ob >> (8 * i)) & 0xffu);
            pcr[c0 + i] = (uint8_t)((orr >> (8 * i)) & 0xffu);
        }
}

template <int PLANAR>
void launch_to_rgb(int sampling, dim3 grid, hipStream_t s, const RgbOp &P) {
    switch (sampling) {
    case HVC_YUV_420: hipLaunchKernelGGL((k_ycc_to_rgb<420, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_422: hipLaunchKernelGGL((k_ycc_to_rgb<422, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_444: hipLaunchKernelGGL((k_ycc_to_rgb<444, PLANAR>), grid, dim3(256), 0, s, P); break;
    default: hipLaunchKernelGGL((k_ycc_to_rgb<400, PLANAR>), grid, dim3(256), 0, s, P); break;
    }
}
template <int PLANAR>
void launch_to_ycc(int sampling, dim3 grid, hipStream_t s, const RgbOp &P) {
    switch (sampling) {
    case HVC_YUV_420: hipLaunchKernelGGL((k_rgb_to_ycc<420, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_422: hipLaunchKernelGGL((k_rgb_to_ycc<422, PLANAR>), grid, dim3(256), 0, s, P); break;
    case HVC_YUV_444: hipLaunchKernelGGL((k_rgb_to_ycc<444, PLANAR>), grid, dim3(256), 0, s, P); break;
    default: hipLaunchKernelGGL((k_rgb_to_ycc<400, PLANAR>), grid, dim3(256), 0, s, P); break;
    }
}

bool is_sampling(int s) { return s == HVC_YUV_420 || s == HVC_YUV_422 || s == HVC_YUV_444 || s == HVC_YUV_400; }

// either direction on device memory, in launches of at most 65535 frames (the grid's second dimension)
hipError_t launch_colour(bool to_rgb, const uint8_t *yuv, size_t yuv_fs, const hvc_component *comps, int sampling, int w, int h, int cw,
                         int ch, int n_frames, const uint8_t *rgb, const RgbImage &im, hipStream_t s) {
    if (n_frames <= 0 || w <= 0 || h <= 0) return hipSuccess;
    const bool grey = sampling == HVC_YUV_400;
    RgbOp P;
    std::memset(&P, 0, sizeof P);
    P.w = w, P.h = h, P.cw = cw, P.ch = ch;
    P.y_stride = comps[0].stride;
    P.cb_stride = grey ? 0 : comps[1].stride, P.cr_stride = grey ? 0 : comps[2].stride;
    P.yuv_fs = yuv_fs;
    P.row_stride = im.row_stride, P.frame_stride = im.frame_stride, P.plane_stride = im.row_stride * (size_t)h;
    const unsigned lrows = sampling == HVC_YUV_420 ? (unsigned)(to_rgb ? (h + 1) >> 1 : h >> 1) : (unsigned)h;
    const unsigned long long lanes = (unsigned long long)((w + 7) >> 3) * lrows;
    if (lanes == 0) return hipSuccess;
    for (int f0 = 0; f0 < n_frames; f0 += 65535) {
        const int cnt = n_frames - f0 < 65535 ? n_frames - f0 : 65535;
        uint8_t *base = const_cast<uint8_t *>(yuv) + (size_t)f0 * yuv_fs;
        P.y = base + comps[0].plane_offset;
        P.cb = grey ? nullptr : base + comps[1].plane_offset;
        P.cr = grey ? nullptr : base + comps[2].plane_offset;
        P.rgb = const_cast<uint8_t *>(rgb) + (size_t)f0 * im.frame_stride;
        const size_t ca = sampling == HVC_YUV_444 ? 8 : 4;
        P.vec_y = ((uintptr_t)P.y | P.y_stride | yuv_fs) % 8 == 0;
        P.vec_c = !grey && ((uintptr_t)P.cb | (uintptr_t)P.cr | P.cb_stride | P.cr_stride | yuv_fs) % ca == 0;
        P.vec_rgb = ((uintptr_t)P.rgb | P.row_stride | P.frame_stride | (im.layout == HVC_RGB_PLANAR ? P.plane_stride : 0)) % 8 == 0;
        const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)cnt, 1);
        if (to_rgb) {
            if (im.layout == HVC_RGB_PLANAR) launch_to_rgb<1>(sampling, grid, s, P);
            else launch_to_rgb<0>(sampling, grid, s, P);
        } else {
            if (im.layout == HVC_RGB_PLANAR) launch_to_ycc<1>(sampling, grid, s, P);
            else launch_to_ycc<0>(sampling, grid, s, P);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace

// bytes of the planes of one frame record that the colour pass touches: [0, span)
size_t rgb_yuv_span(const hvc_component *comps, int sampling, int w, int h, int cw, int ch) {
    size_t span = comps[0].plane_offset + (size_t)(h - 1) * comps[0].stride + (size_t)w;
    for (int k = 1; k < 3 && sampling != HVC_YUV_400; k++)
        span = std::max(span, comps[k].plane_offset + (size_t)(ch - 1) * comps[k].stride + (size_t)cw);
    return span;
}

// the arguments every entry point shares: HVC_OK with *nothing = true when there is nothing to write
int rgb_check_args(const hvc_ctx *c, int sampling, int width, int height, int n_frames, int layout, int where, size_t rgb_row_stride,
                 size_t rgb_frame_stride, RgbImage &im, bool &nothing) {
    if (!c || !is_sampling(sampling) || width < 0 || height < 0 || n_frames < 0) return HVC_E_INVALID_ARG;
    if (where != HVC_MEM_HOST && where != HVC_MEM_DEVICE) return HVC_E_INVALID_ARG;
    if (!rgb_image(layout, width, height, rgb_row_stride, rgb_frame_stride, im)) return HVC_E_INVALID_ARG;
    if (width > (1 << 24) || height > (1 << 24) || (unsigned long long)((width + 7) / 8) * (unsigned long long)height >= (1ull << 31)) return HVC_E_TOO_LARGE;
    nothing = width == 0 || height == 0 || n_frames == 0;
    return HVC_OK;
}


bool rgb_image(int layout, int width, int height, size_t row_stride, size_t frame_stride, RgbImage &im) {
    if (layout != HVC_RGB_INTERLEAVED && layout != HVC_RGB_PLANAR) return false;
    const size_t tight_row = layout == HVC_RGB_PLANAR ? (size_t)width : (size_t)3 * width;
    im.layout = layout;
    im.row_bytes = tight_row;
    im.rows = layout == HVC_RGB_PLANAR ? (size_t)3 * height : (size_t)height; // (planar planes are row_stride * height apart: 3 h rows)
    im.row_stride = row_stride ? row_stride : tight_row;
    if (im.row_stride < tight_row) return false;
    const size_t tight_frame = im.row_stride * im.rows;
    im.frame_stride = frame_stride ? frame_stride : tight_frame;
    return im.frame_stride >= tight_frame;
}

int rgb_sampling_of(const hvc_jpeg_info &info) {
    if (info.n_comp == 1) return HVC_YUV_400;
    if (info.n_comp != 3) return 0;
    const hvc_jpeg_component *k = info.comp;
    if (k[1].hscale != k[2].hscale || k[1].vscale != k[2].vscale || k[1].hscale < 1 || k[1].vscale < 1) return 0;
    if (k[0].hscale == k[1].hscale && k[0].vscale == k[1].vscale) return HVC_YUV_444;
    if (k[0].hscale == 2 * k[1].hscale && k[0].vscale == 2 * k[1].vscale) return HVC_YUV_420;
    if (k[0].hscale == 2 * k[1].hscale && k[0].vscale == k[1].vscale) return HVC_YUV_422;
    return 0;
}

void rgb_chroma_window(int sampling, int width, int height, int &cw, int &ch) {
    cw = sampling == HVC_YUV_444 ? width : (width + 1) / 2;
    ch = sampling == HVC_YUV_420 ? (height + 1) / 2 : height;
}

hipError_t ycc_to_rgb_device(const uint8_t *d_yuv, size_t yuv_fs, const hvc_component *comps, int sampling, int width, int height, int cw,
                             int ch, int n_frames, uint8_t *d_rgb, const RgbImage &im, hipStream_t s) {
    return launch_colour(true, d_yuv, yuv_fs, comps, sampling, width, height, cw, ch, n_frames, d_rgb, im, s);
}
hipError_t rgb_to_ycc_device(const uint8_t *d_rgb, const RgbImage &im, int width, int height, int sampling, int n_frames, uint8_t *d_yuv,
                             size_t yuv_fs, const hvc_component *comps, hipStream_t s) {
    return launch_colour(false, d_yuv, yuv_fs, comps, sampling, width, height, 0, 0, n_frames, d_rgb, im, s);
}
hipError_t rgb_download(const uint8_t *d_rgb, uint8_t *h_rgb, const RgbImage &im, int n_frames, hipStream_t s) {
    if (im.row_stride == im.row_bytes && im.frame_stride == im.row_stride * im.rows)
        return hipMemcpyAsync(h_rgb, d_rgb, im.frame_stride * (size_t)n_frames, hipMemcpyDeviceToHost, s);
    for (int f = 0; f < n_frames; f++) { // (only what was written: the caller's padding stays)
        const hipError_t e = hipMemcpy2DAsync(h_rgb + (size_t)f * im.frame_stride, im.row_stride, d_rgb + (size_t)f * im.frame_stride,
                                              im.row_stride, im.row_bytes, im.rows, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
size_t rgb_bytes(const RgbImage &im, int n_frames) { // from the first byte to the last one written
    return n_frames < 1 || !im.rows ? 0 : (size_t)(n_frames - 1) * im.frame_stride + (im.rows - 1) * im.row_stride + im.row_bytes;
}
