// hvc_fancy_dev.h -- device side of the colour pass with libjpeg's "fancy" upsampling (internal): the lane k_ycc_to_rgb_fancy
// (hvc_libjpeg.hip, one geometry per launch) and k_ycc_to_rgb_fancy_mixed (hvc_mixed_libjpeg.hip, geometry per wavefront from
// device memory) share.  Loads of Y, colour matrix and stores are hvc_rgb_dev.h's; what the triangle filter is and why its
// neighbours are byte loads is said at the top of hvc_libjpeg.hip.  Everything here has internal linkage: include it in a
// .hip file only.
#ifndef HVC_FANCY_DEV_H
#define HVC_FANCY_DEV_H

#include "hvc_rgb_dev.h"

namespace {

// samples c0 - 1 .. c0 + 4 of a chroma row of n valid samples, clamped to the row's window [0, n - 1]; c0 < n
__device__ __forceinline__ void load6(const uint8_t *row, int c0, int n, bool vec, int (&s)[6]) {
    unsigned a, nb;
    load4n(row, c0, n, vec, a, nb);
    s[0] = (int)row[max(c0 - 1, 0)];
#pragma unroll
    for (int i = 0; i < 4; i++) s[1 + i] = (int)((a >> (8 * i)) & 0xffu);
    s[5] = (int)(nb >> 24);
}
// the triangle filter along a row: t[0..5] = positions c0 - 1 .. c0 + 4 -> the 8 samples 2 c0 .. 2 c0 + 7
__device__ __forceinline__ void fancy_h(const int (&t)[6], int r0, int r1, int sh, unsigned &lo, unsigned &hi) {
    unsigned o[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned e = (unsigned)((3 * t[i + 1] + t[i] + r0) >> sh), d = (unsigned)((3 * t[i + 1] + t[i + 2] + r1) >> sh);
        o[i >> 1] |= (e | d << 8) << (16 * (i & 1));
    }
    lo = o[0], hi = o[1];
}

// One lane of planes -> RGB with the triangle filter, spelled inline in its kernel (a macro for the reason hvc_rgb_dev.h gives
// at HVC_YCC_LANE_TO_RGB): columns 8 g .. 8 g + 7 of lane row lr of frame f of P (one frame per P: f = 0).  S (420, 422, 444 or
// 400 = luma only) and PLANAR are compile-time constants of the scope that expands it.  (P).cw x (P).ch is the chroma WINDOW
// the filter clamps to; a window at most 2 samples wide is replicated (libjpeg picks its plain routine there): an
// image-uniform branch.
#define HVC_YCC_LANE_TO_RGB_FANCY(P, f, lr, g) \
    do { \
        constexpr int ROWS = S == 420 ? 2 : 1; \
        const int x0 = (int)(8 * (g)); \
        const bool full = x0 + 8 <= (P).w; \
        unsigned cb[ROWS][2], cr[ROWS][2]; \
        if (S == 444) { \
            load8((P).cb + (f) * (P).yuv_fs + (size_t)(lr) * (P).cb_stride, x0, (P).cw, (P).vec_c && full, cb[0][0], cb[0][1]); \
            load8((P).cr + (f) * (P).yuv_fs + (size_t)(lr) * (P).cr_stride, x0, (P).cw, (P).vec_c && full, cr[0][0], cr[0][1]); \
        } else if (S != 400) { \
            const int c0 = (int)(4 * (g)); /* (8 g < w, so c0 < ceil(w / 2) <= cw) */ \
            const bool vc = (P).vec_c && c0 + 4 <= (P).cw; \
            _Pragma("unroll") for (int k = 0; k < 2; k++) { \
                const uint8_t *plane = (k ? (P).cr : (P).cb) + (f) * (P).yuv_fs; \
                const size_t stride = k ? (P).cr_stride : (P).cb_stride; \
                unsigned(*out)[2] = k ? cr : cb; \
                const uint8_t *row = plane + (size_t)(lr) * stride; \
                if ((P).cw <= 2) { /* plain replication, 2x or 2x2 */ \
                    unsigned a, an; \
                    load4n(row, c0, (P).cw, vc, a, an); \
                    interleave(a, a, out[0][0], out[0][1]); \
                    out[ROWS - 1][0] = out[0][0], out[ROWS - 1][1] = out[0][1]; \
                    continue; \
                } \
                int s[6]; \
                load6(row, c0, (P).cw, vc, s); \
                if (S == 422) { \
                    fancy_h(s, 1, 2, 2, out[0][0], out[0][1]); \
                } else { \
                    int up[6], dn[6]; \
                    load6(plane + (size_t)((lr) ? (lr) - 1u : 0u) * stride, c0, (P).cw, vc, up); \
                    load6(plane + (size_t)min((lr) + 1u, (unsigned)(P).ch - 1u) * stride, c0, (P).cw, vc, dn); \
                    _Pragma("unroll") for (int i = 0; i < 6; i++) { \
                        up[i] += 3 * s[i]; \
                        dn[i] += 3 * s[i]; \
                    } \
                    fancy_h(up, 8, 7, 4, out[0][0], out[0][1]); \
                    fancy_h(dn, 8, 7, 4, out[ROWS - 1][0], out[ROWS - 1][1]); \
                } \
            } \
        } \
        uint8_t *frame = (P).rgb + (f) * (P).frame_stride; \
        _Pragma("unroll") for (int rr = 0; rr < ROWS; rr++) { \
            const int row = (int)(lr) * ROWS + rr; \
            if (row >= (P).h) break; \
            unsigned y[2], r[2], gg[2], b[2]; \
            load8((P).y + (f) * (P).yuv_fs + (size_t)row * (P).y_stride, x0, (P).w, (P).vec_y && full, y[0], y[1]); \
            if (S == 400) { \
                r[0] = gg[0] = b[0] = y[0]; \
                r[1] = gg[1] = b[1] = y[1]; \
            } else { \
                ycc4_to_rgb(y[0], cb[rr][0], cr[rr][0], r[0], gg[0], b[0]); \
                ycc4_to_rgb(y[1], cb[rr][1], cr[rr][1], r[1], gg[1], b[1]); \
            } \
            store_rgb<PLANAR>((P), frame, row, x0, (P).vec_rgb && full, r, gg, b); \
        } \
    } while (0)

} // namespace
#endif
