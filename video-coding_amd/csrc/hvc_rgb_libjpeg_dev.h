// hvc_rgb_libjpeg_dev.h -- one lane of the libjpeg-exact colour pass RGB -> Y, Cb, Cr (hvc_set_encode_libjpeg; include/hvc_jpeg.h
// "Encoding bit-exact to libjpeg", 4), expanded by k_rgb_to_ycc_libjpeg and k_rgb_to_ycc_libjpeg_mixed (hvc_libjpeg_encode.hip).
//
// A lane makes 8 luma columns of one row -- of two rows under 4:2:0 -- and the chroma samples under them: 4 columns under
// 4:2:0 / 4:2:2, so the lane's first chroma column is a multiple of 4 and the alternating bias of jcsample.c depends on the
// position inside the lane alone: h2v2 (a + b + c + d + 1 + (j & 1)) >> 2, h2v1 (a + b + (j & 1)) >> 1 for the lane's j-th.
// The colour step is the existing libjpeg form (tools/rgb_reference.py holds it to libjpeg-turbo on all 2^24 inputs).
//
// Edges.  The lane works in the coordinates of the OUTPUT planes and clamps what it reads: a full-size column past the image
// is the last column (jcsample.c expand_right_edge: BEFORE the averaging, so a padded chroma column is not always the copy of
// the last real one); a luma row past the image is the last row; a chroma row past the last one is the last AVERAGED row
// (jcprepct.c).  How far it writes is the caller's: the frame's own samples (hvc_rgb_to_yuv, hvc_rgb_to_yuv_mixed: planes that
// may have no room for more), or every component up to ceil(actual / 8) * 8 both ways (`pad`: the encode pipelines, whose
// planes are whole blocks -- the replicated edge the block stage needs; what lies beyond are dummy blocks).
#ifndef HVC_RGB_LIBJPEG_DEV_H
#define HVC_RGB_LIBJPEG_DEV_H

#include <hip/hip_runtime.h>

#include "hvc_mixed_rgb_plan.h"

namespace hvc {

__device__ __forceinline__ int lje_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int lje_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int lje_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// 8 pixels of image row `row` from column x0, columns clamped to w - 1, as r[], g[], b[]
__device__ __forceinline__ void lje_load_row(const MixedRgbImageK &K, const uint8_t *rgb, bool planar, int row, int x0, int (&r)[8],
                                             int (&g)[8], int (&b)[8]) {
    const uint8_t *p = rgb + K.rgb_base + (size_t)row * K.row_stride;
    if (planar) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int x = min(x0 + i, K.w - 1);
            r[i] = p[x];
            g[i] = p[K.plane_stride + x];
            b[i] = p[2 * K.plane_stride + x];
        }
        return;
    }
    const uint8_t *q = p + (size_t)3 * x0;
    if (x0 + 8 <= K.w && ((uintptr_t)q & 3) == 0) { // the lane's 24 bytes as six dwords
        unsigned d[6];
#pragma unroll
        for (int k = 0; k < 6; k++) d[k] = reinterpret_cast<const unsigned *>(q)[k];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            r[i] = (int)((d[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 0xffu);
            g[i] = (int)((d[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 0xffu);
            b[i] = (int)((d[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 0xffu);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int x = min(x0 + i, K.w - 1);
        r[i] = p[3 * x];
        g[i] = p[3 * x + 1];
        b[i] = p[3 * x + 2];
    }
}

// n <= 8 samples v[] to row address `dst` from column x0, columns below `ext` only: one 8- or 4-byte store where it is whole
// and aligned
template <int N>
__device__ __forceinline__ void lje_store(uint8_t *dst, int x0, int ext, const int (&v)[8]) {
    uint8_t *p = dst + x0;
    if (x0 + N <= ext && ((uintptr_t)p & (N - 1)) == 0) {
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) lo |= (unsigned)v[i] << (8 * i);
        if (N == 8) {
#pragma unroll
            for (int i = 0; i < 4; i++) hi |= (unsigned)v[4 + i] << (8 * i);
            typedef unsigned u2v __attribute__((ext_vector_type(2)));
            const u2v t = {lo, hi};
            *reinterpret_cast<u2v *>(p) = t;
        } else {
            *reinterpret_cast<unsigned *>(p) = lo;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < N; i++)
        if (x0 + i < ext) p[i] = (uint8_t)v[i];
}

// lane: the lane's index inside the image (K.groups lanes a lane row: hvc_libjpeg_encode_plan.h libjpeg_rgb_plan_lanes)
__device__ __forceinline__ void rgb_to_ycc_libjpeg_lane(const MixedRgbImageK &K, unsigned lane, const uint8_t *rgb, uint8_t *yuv, bool planar,
                                                        bool pad) {
    const unsigned ly = K.groups == 1 ? lane : __umulhi(lane, K.magic);
    const int lx = (int)(lane - ly * K.groups), x0 = 8 * lx;
    const bool sub_h = K.sampling == HVC_YUV_420 || K.sampling == HVC_YUV_422, sub_v = K.sampling == HVC_YUV_420;
    const bool grey = K.sampling == HVC_YUV_400;
    const int cw = sub_h ? K.w / 2 : K.w, ch = sub_v ? K.h / 2 : K.h; // the frame's own chroma samples (even sizes where sub-sampled)
    const int ewy = pad ? (K.w + 7) & ~7 : K.w, ehy = pad ? (K.h + 7) & ~7 : K.h;
    const int ewc = pad ? (cw + 7) & ~7 : cw, ehc = pad ? (ch + 7) & ~7 : ch;
    const int rows = sub_v ? 2 : 1;
    int sb[8], sr[8]; // chroma of the 8 full-size columns, summed over the lane's rows
#pragma unroll
    for (int i = 0; i < 8; i++) sb[i] = sr[i] = 0;
    const int crow = sub_v ? (int)ly : 0; // (4:2:0) the chroma row, and the one its samples are averaged for
    const int csrc = min(crow, ch - 1);
    for (int k = 0; k < rows; k++) {
        const int y = (int)ly * rows + k;              // luma row of the output
        const int ys = min(y, K.h - 1);                // ... and the image row it shows
        const int yc = sub_v ? 2 * csrc + k : ys;      // the image row the chroma of this pass is made from
        int r[8], g[8], b[8];
        lje_load_row(K, rgb, planar, ys, x0, r, g, b);
        if (y < ehy) {
            int v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = lje_y(r[i], g[i], b[i]);
            lje_store<8>(yuv + K.y_base + (size_t)y * K.y_stride, x0, ewy, v);
        }
        if (grey) continue;
        if (yc != ys) lje_load_row(K, rgb, planar, yc, x0, r, g, b);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            sb[i] += lje_cb(r[i], g[i], b[i]);
            sr[i] += lje_cr(r[i], g[i], b[i]);
        }
    }
    if (grey) return;
    const int cy = sub_v ? crow : (int)ly;
    if (cy >= ehc) return;
    uint8_t *pb = yuv + K.cb_base + (size_t)cy * K.cb_stride, *pr = yuv + K.cr_base + (size_t)cy * K.cr_stride;
    int vb[8], vr[8];
    if (sub_h) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int bias = sub_v ? 1 + (j & 1) : (j & 1), sh = sub_v ? 2 : 1;
            vb[j] = (sb[2 * j] + sb[2 * j + 1] + bias) >> sh;
            vr[j] = (sr[2 * j] + sr[2 * j + 1] + bias) >> sh;
            vb[4 + j] = vr[4 + j] = 0;
        }
        lje_store<4>(pb, 4 * lx, ewc, vb);
        lje_store<4>(pr, 4 * lx, ewc, vr);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) vb[i] = sb[i], vr[i] = sr[i];
        lje_store<8>(pb, x0, ewc, vb);
        lje_store<8>(pr, x0, ewc, vr);
    }
}

} // namespace hvc
#endif
